// The derived weight forms of a conv.  The fast kernels do not read a layer's weights w [Cin][KK][CoutPad] but copies made from them; this
// header is the one place that says which layer holds which copy, how large it is and what it is made from (form_spec), which of the held
// copies a launch may read (select_fwd_forms / select_dgrad_forms), and how a descriptor table of a batched refresh reaches the device
// (DescTable).  A new form is a FormId, a case of form_spec and a line of the selection; model.hip's hold_form / fill_form do the rest for
// the handle and for the test hooks alike.
#pragma once
#include <vector>

#include "kernels.h"

namespace vr {

// forward: U = G g G^T, U as three bf16 planes, w as bf16 x 3 (mfma_mode 2) or fp16 x 2 + scale tails (mode 3) in ONE buffer;
// data gradient: the flipped / transposed wt [Cout][KK][CinPad], the same three forms of wt, the four parity classes of a stride-2 3x3
enum FormId { F_WINO = 0, F_WINO6, F_X3W, F_WT, F_WINOT, F_WINOT6, F_X3T, F_S2W, F_COUNT };

// What a layer's shape makes it, set once where the layer is built: a plain 3x3 stride-1 conv (conv_wino / conv_x3 / conv_x3h), a
// conv_x3d.hip layer (dilated 3x3, or a 1x1 the caller names a branch: the handle names aspp.conv2, the hooks any 1x1), a 3x3 stride-2
// conv (conv_x3s.hip, parity-class data gradient), or none of them.
enum FormClass { FC_NONE = 0, FC_PLAIN3, FC_X3D, FC_S2 };
inline FormClass form_class(int ks, int stride, int dh, int dw, bool branch_1x1) {
    if (ks == 3 && stride == 1 && dh == 1 && dw == 1) return FC_PLAIN3;
    if (stride == 1 && ((ks == 3 && dh > 1) || (ks == 1 && branch_1x1))) return FC_X3D;
    if (ks == 3 && stride == 2 && dh == 1 && dw == 1) return FC_S2;
    return FC_NONE;
}

// one slot per form, null when the layer does not hold it
struct WeightForms {
    void* p[F_COUNT] = {};
    float* f32(FormId f) const { return static_cast<float*>(p[f]); }
};

// who gets the bf16 planes of U: nobody, the layers whose padded output count is a multiple of 64 (the handle, under VR_CONV_X3=0: only
// conv_wino's 64-cout variant reads them), or every plain layer (the forward hooks in mfma_mode 2)
enum Wino6Want { W6_NONE = 0, W6_PAD64, W6_ALL };

// the planes of w / wt: a plain 3x3 is split in modes 2 and 3, the other classes have fp16 kernels only (mode 3)
inline bool planes_live(FormClass cls, int mfma_mode) { return cls == FC_PLAIN3 ? (mfma_mode == 2 || mfma_mode == 3) : mfma_mode == 3; }

// THE RULE.  held: the layer has a buffer for the form (whatever the mode: the one buffer holds the image of the current mode);
// live: mfma_mode fills and reads it; from_wt: made from the layer's wt, not from w; (rows, KK, pad): the dims of its descriptor.
struct FormSpec { bool held, live, from_wt; size_t bytes; int rows, KK, pad; };
inline FormSpec form_spec(FormId f, FormClass cls, int Cin, int Cout, int KK, int CoutPad, int mfma_mode, Wino6Want w6) {
    const int CinPad = (Cin + 31) / 32 * 32;
    const bool plain = cls == FC_PLAIN3;
    auto six = [&](int pad) { return plain && (w6 == W6_ALL || (w6 == W6_PAD64 && pad % 64 == 0)); };
    switch (f) {
    case F_WINO:   return {plain, true, false, (size_t)Cin * 16 * CoutPad * 4, Cin, 9, CoutPad};
    case F_WINO6:  return {six(CoutPad), mfma_mode == 2, false, wino_weights6_bytes(Cin, CoutPad), Cin, 9, CoutPad};
    case F_X3W:    return {cls != FC_NONE, planes_live(cls, mfma_mode), false, x3_weights_bytes(Cin, KK, CoutPad), Cin, KK, CoutPad};
    case F_WT:     return {true, true, false, (size_t)Cout * KK * CinPad * 4, Cout, KK, CinPad};
    case F_WINOT:  return {plain, true, true, (size_t)Cout * 16 * CinPad * 4, Cout, 9, CinPad};
    case F_WINOT6: return {six(CinPad), mfma_mode == 2, true, wino_weights6_bytes(Cout, CinPad), Cout, 9, CinPad};
    case F_X3T:    return {plain || cls == FC_X3D, planes_live(cls, mfma_mode), true, x3_weights_bytes(Cout, KK, CinPad), Cout, KK, CinPad};
    default:       return {cls == FC_S2, true, false, (size_t)4 * Cout * 9 * CinPad * 4, Cout, 9, CinPad};
    }
}

// Which of the held forms a launch may read: the handle's state at the launch (the forward hooks launch as an eval call does).
struct FormSelect { int mfma_mode; bool training, train_wino; int x3d_mode, x3s_mode; bool dry; };

inline void select_fwd_forms(ConvArgs& a, const WeightForms& F, const FormSelect& s, int Win, int stride) {
    const bool fp32_train = s.training && !s.train_wino;     // option train_winograd 0: the direct fp32 kernels
    a.wino = fp32_train ? nullptr : F.f32(F_WINO);           // (null until the first refresh)
    a.wino6 = (a.wino && s.mfma_mode == 2) ? F.p[F_WINO6] : nullptr;
    a.x3w = ((s.mfma_mode == 2 || s.mfma_mode == 3) && !fp32_train) ? F.p[F_X3W] : nullptr;
    if (!s.x3d_mode && Win == 16) a.x3w = nullptr;           // (16-column layers: only conv_x3d.hip reads the planes)
    if (stride == 2 && (s.training || !s.x3s_mode)) a.x3w = nullptr;   // (conv_x3s.hip is eval only; option conv_x3s 0: conv_dma.hip)
}

// ... of the data gradient of a layer of class `cls`; a dry (planning) pass sets none.  The parity-class weights are not a ConvArgs form:
// bwd_conv_dgrad reads F.p[F_S2W] itself.
inline void select_dgrad_forms(ConvArgs& d, const WeightForms& F, FormClass cls, const FormSelect& s, int Win) {
    const bool fast = !s.dry && s.train_wino;
    d.w = s.dry ? nullptr : F.f32(F_WT);
    d.wino = fast ? F.f32(F_WINOT) : nullptr;
    d.wino6 = (d.wino && s.mfma_mode == 2) ? F.p[F_WINOT6] : nullptr;
    d.x3w = (fast && planes_live(cls, s.mfma_mode)) ? F.p[F_X3T] : nullptr;
    if (!s.x3d_mode && Win == 16) d.x3w = nullptr;
}

inline bool operator==(const WinoWDesc& a, const WinoWDesc& b) { return a.w == b.w && a.u == b.u && a.Cin == b.Cin && a.CoutPad == b.CoutPad; }
inline bool operator==(const X3WDesc& a, const X3WDesc& b) { return a.w == b.w && a.o == b.o && a.Cin == b.Cin && a.KK == b.KK && a.CoutPad == b.CoutPad; }
inline bool operator==(const FlipDesc& a, const FlipDesc& b) { return a.w == b.w && a.wt == b.wt && a.Cin == b.Cin && a.Cout == b.Cout && a.KK == b.KK; }
inline bool operator==(const S2WDesc& a, const S2WDesc& b) { return a.w == b.w && a.wc == b.wc && a.Cin == b.Cin && a.Cout == b.Cout; }

// The descriptor table of a batched launch: host copy + device copy, re-uploaded only when the table changed.
template <class D>
struct DescTable {
    std::vector<D> host;
    D* dev = nullptr;
    const D* upload(const std::vector<D>& descs, hipStream_t st) {
        if (dev && descs == host) return dev;
        VR_HIP(hipStreamSynchronize(st));                    // (a launch may still read the old table)
        if (dev) VR_HIP(hipFree(dev));
        dev = nullptr;
        VR_HIP(hipMalloc(reinterpret_cast<void**>(&dev), descs.size() * sizeof(D)));
        VR_HIP(hipMemcpy(dev, descs.data(), descs.size() * sizeof(D), hipMemcpyHostToDevice));
        host = descs;
        return dev;
    }
    void release() { (void)hipFree(dev); dev = nullptr; host.clear(); }
};

// What a set of convs holds: one allocation per form and the tables of its refresh launches (a form uses the table of its descriptor type).
struct FormStore {
    char* arena[F_COUNT] = {};
    struct Tables {
        DescTable<WinoWDesc> wino; DescTable<X3WDesc> x3; DescTable<FlipDesc> flip; DescTable<S2WDesc> s2;
        int mode = -1, n = 0, max_cout_pad = 0;               // the mfma_mode the table was made for, its layers and grid sizes
        long long max_elems = 0;
    } tbl[F_COUNT];
    void release() {
        for (int f = 0; f < F_COUNT; ++f) {
            (void)hipFree(arena[f]); arena[f] = nullptr;
            tbl[f].wino.release(); tbl[f].x3.release(); tbl[f].flip.release(); tbl[f].s2.release();
        }
    }
};

}  // namespace vr
