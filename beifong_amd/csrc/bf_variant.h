// Which instantiation of bf_render_kernel (bf_kernels.hip) a launch runs: the kernel variant word (bf_device.h) as a pure function of
// the launch's shape and its integrator feature.  Plain C++ with no HIP in it, so that a host-only program can include it
// (tests/native/variant_check.cpp walks every combination); render_launch and tail_launch turn the word into the instantiation.
#pragma once

namespace bfv {
// the bits of bf_device.h's variant word (bf_kernels.hip asserts that they are the same numbers)
constexpr int kWide = 4, kLean = 8, kMulti = 16, kGeom = 32, kMoment = 64, kClass = 128, kAov = 256, kSum = 512;
// tail only: the two-waves-per-SIMD build of the general kernel, <S, true, P, 2>; never with a variant bit
constexpr int kTailTwo = 1 << 16;
constexpr int kInvalid = -1;      // the launch is refused (hipErrorInvalidValue)

enum Feature { kPlain = 0, kFeatMoment = 1, kFeatClass = 2, kFeatAov = 3, kFeatSum = 4 };      // which family of launchers was called

struct Shape {
    bool geom;             // DLaunch::geom_stride != 0
    bool wide, lean, multi, roll;      // DLaunch's words of those names, != 0
    bool receive_raw;      // DLaunch::mode == BF_MODE_RECEIVE_RAW
    bool two;              // tail only: tail_waves == 2
};

// the forms the class and AOV kernels and the one-kernel render come in: a lean scene runs the general kernel
inline int general_form(const Shape &s) { return (s.geom ? kGeom : 0) | (s.wide ? kWide : 0); }

// the one-kernel render (RESUME = false)
inline int render_variant(Feature f, const Shape &s) {
    switch (f) {
        case kFeatMoment: return kMoment | general_form(s);
        case kFeatClass: return kClass | general_form(s);
        case kFeatAov: return (s.receive_raw || s.roll) ? kInvalid : (kAov | general_form(s));
        case kFeatSum: return (s.multi || s.roll) ? kInvalid : (kSum | general_form(s));
        default: return general_form(s);
    }
}

// the wavefront tail (RESUME = true).  Per-render geometry takes the wide or else the lean form with it; per-path tables (multi)
// come before wide, wide before lean.  The moment tail is three waves per SIMD whatever tail_waves says; the plain tail is lean
// only with three, and takes the two-wave build only when no variant bit applies.
inline int tail_variant(Feature f, const Shape &s) {
    if (f == kFeatClass) return (s.multi || s.roll) ? kInvalid : (kClass | general_form(s));
    if (f == kFeatAov) return (s.receive_raw || s.roll) ? kInvalid : (kAov | general_form(s));
    if (f == kFeatSum) return (s.multi || s.roll) ? kInvalid : (kSum | general_form(s));
    const int m = f == kFeatMoment ? kMoment : 0;
    if (s.geom) return m | kGeom | (s.wide ? kWide : (s.lean ? kLean : 0));
    if (s.multi) return m | kMulti;
    if (s.wide) return m | kWide;
    if (f == kFeatMoment) return m | (s.lean ? kLean : 0);
    if (s.lean && !s.two) return kLean;
    return s.two ? kTailTwo : 0;
}
}  // namespace bfv
