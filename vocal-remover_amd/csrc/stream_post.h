// spec_utils.merge_artifacts (lib/spec_utils.py:60-93) in incremental form, for streams.  One piece of code for the
// host (vr_debug_stream_post_weight) and the device (the walk of frame_min_kernel's stream form, stft.hip).
//
// Offline (merge_artifacts_weight, model.hip) the blend weight of every frame comes from the runs of frames whose mask minimum is above
// `thres`: a run [s0, e0] with e0 - s0 > M is an artifact; if it begins less than F frames behind the previous artifact's end old_e, its
// start moves back to old_e - 2F; it writes a ramp up on [s, s + F), ones on [s + F, e0 - F), a ramp down on [e0 - F, e0).  Here the minima
// arrive frame by frame and the weights live in a ring, weight of frame t at wgt[t % RW]:
//   - frame h enters with weight 0;
//   - a run is confirmed as an artifact by its frame s0 + M + 1: the ramp up is written then, and the ones up to F + 1 frames below
//     the confirming frame (the run is known to reach it, so these are ones whatever follows);
//   - every further frame t of a confirmed run makes frame t - F - 1 a one;
//   - the frame that ends the run (or the flush) writes the ramp down.
// The earliest frame a step can rewrite is the moved-back start of a run confirmed by the step's last frame h1 - 1, s0 - 3F + 1 =
// h1 - (3F + M + 1): weight[t] is final once the minima of the frames below t + kStreamPostDelay are known, and not before.  The
// schedule counts frames and declares the h1 - kStreamPostDelay frames below that one final (one frame in hand).  A ring of
// RW >= kStreamPostDelay + (frames of the largest step) entries never overwrites a frame that is still read.  The song's length enters
// nowhere: `e0 != T` of the reference always holds (e0 <= T - 1) and its negative-index wrap cannot happen (old_e - 2F >= 1).
// The one deviation: no frame above the threshold is the reference's IndexError; here it is all zeros (no blend).
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VR_POST_HD __host__ __device__ inline
#else
#define VR_POST_HD inline
#endif

namespace vr {

constexpr float kStreamPostThres = 0.05f;            // the constants of Model::separate_run
constexpr int kStreamPostMinRange = 64;
constexpr int kStreamPostFade = 32;
constexpr int kStreamPostDelay = 3 * kStreamPostFade + kStreamPostMinRange + 1;     // 161
static_assert(kStreamPostMinRange >= 2 * kStreamPostFade, "min_range must be >= fade_size * 2");

// All zero = the state before frame 0 (the stream's slab is zeroed at open).
struct StreamPostState {
    int h;              // the next frame
    int open;           // 1 + the first frame of the run the last frame belongs to; 0: the last frame is below the threshold
    int confirmed;      // the open run is an artifact: its ramp up is written
    int have_old;       // an artifact run has ended
    int old_e;          // ... with this last frame
};

// the floats merge_artifacts_weight writes: np.linspace(0, 1, F)[i] and np.linspace(1, 0, F)[i]
VR_POST_HD float stream_post_ramp(int i, bool up) {
    const double x = (double)i / (kStreamPostFade - 1);
    return (float)(up ? x : 1.0 - x);
}

// the run that ends with frame e0: an artifact leaves its ramp down
VR_POST_HD void stream_post_close(StreamPostState& s, int e0, float* wgt, int RW) {
    if (s.confirmed) {
        for (int i = 0; i < kStreamPostFade; ++i) wgt[(e0 - kStreamPostFade + i) % RW] = stream_post_ramp(i, false);
        s.have_old = 1;
        s.old_e = e0;
    }
    s.open = 0;
    s.confirmed = 0;
}

// Takes the minima of the frames [s.h, s.h + n): fmin[i] belongs to frame s.h + i.  Writes ring entries of frames >= s.h + n -
// kStreamPostDelay only.  (The ring position of frame t moves along with t: one division per call, none per frame -- one lane walks
// this loop on the device.)
VR_POST_HD void stream_post_advance(StreamPostState& s, const float* fmin, int n, float* wgt, int RW) {
    constexpr int F = kStreamPostFade, M = kStreamPostMinRange;
    int slot = s.h % RW;
    for (int i = 0; i < n; ++i) {
        const int t = s.h;
        wgt[slot] = 0.f;
        const int back = slot - F - 1 < 0 ? slot - F - 1 + RW : slot - F - 1;       // frame t - F - 1 (RW > F + 1)
        slot = slot + 1 == RW ? 0 : slot + 1;
        if (fmin[i] > kStreamPostThres) {
            if (!s.open) s.open = t + 1;
            const int s0 = s.open - 1;
            if (!s.confirmed && t - s0 > M) {              // t == s0 + M + 1
                s.confirmed = 1;
                int a = s0;
                if (s.have_old && s0 - s.old_e < F) a = s.old_e - 2 * F;
                int ones = 0;                               // a run from frame 0 has no ramp up: ones from the start
                if (a != 0) {
                    for (int j = 0; j < F; ++j) wgt[(a + j) % RW] = stream_post_ramp(j, true);
                    ones = a + F;
                }
                for (int j = ones; j < t - F - 1; ++j) wgt[j % RW] = 1.f;
            }
            if (s.confirmed) wgt[back] = 1.f;               // the run reaches t: frame t - F - 1 lies below e0 - F
        } else if (s.open) {
            stream_post_close(s, t - 1, wgt, RW);
        }
        s.h = t + 1;
    }
}

// the flush: the open run ends with the last frame; every weight below s.h is final afterwards
VR_POST_HD void stream_post_finish(StreamPostState& s, float* wgt, int RW) {
    if (s.open) stream_post_close(s, s.h - 1, wgt, RW);
}

}  // namespace vr
