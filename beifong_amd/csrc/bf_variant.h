// Which template instantiation a launch runs, as pure functions of the launch's shape and its integrator feature: the kernel variant
// word (bf_device.h) of bf_render_kernel (bf_kernels.hip: render_variant, tail_variant), the <FIRST, W, V> of wf_shade and the
// <STATS, W, SHIFT, QUANT, GEOM> of wf_trace (bf_wavefront.hip: shade_variant, trace_variant), and which of those two kernels'
// instantiations exist (shade_exists, trace_exists: what the launchers instantiate and dispatch over).  Plain C++ with no HIP in it, so
// that a host-only program can include it (tests/native/variant_check.cpp walks every combination) and the render driver can ask what
// a launch will get (bf_render.cpp: wf_setup).
#pragma once

namespace bfv {
// the bits of bf_device.h's variant word (bf_kernels.hip and bf_wavefront.hip assert that they are the same numbers)
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

// ---- wf_shade<FIRST, W, V> ----
// V is the mode class (bit 0: the receive modes) ORed with the variant bits above; first < 0 is a refused launch
struct ShadeForm {
    int first, w, v;
};
constexpr ShadeForm kRefused = {kInvalid, 0, 0};

// The shading launch of family `f` (`fast`: the fast-arithmetic object, which holds the plain family only): `first` is the launch
// kind (0 walk, 1 first launch of a pool, 2 wake launch of a rolling call, 3 evicting walk; Shape::two means nothing here), `waves`
// the register budget the host asks for (waves per SIMD).  Everything runs at three waves but:
//   the general walk (first 0), which has builds at 1 (any other request), 2, 3 and 4;
//   the lean launches that START paths (first 1, and first 2 outside the receive modes), which have a second, scratch-free build at 4
//   (profiles/no_slp_resource_usage.txt; the receive wake launch would spill 20 B per lane, every other form 16-140 B).  THE rule for
//   four waves: wf_setup sizes such a launch's grid by the W it reads here.
// The lean walk exists at three waves only: at another budget a lean scene runs the general kernel.  The class, AOV and exact-sum
// families come in the general forms and are never part of a rolling sequence (first < 2); neither is per-render geometry.
inline ShadeForm shade_variant(Feature f, bool fast, const Shape &s, int first, int waves) {
    if (fast && f != kPlain) return kRefused;
    const int rx = s.receive_raw ? 1 : 0, one = first ? 1 : 0, any = (first == 2 || first == 3) ? first : one;
    if (f == kFeatClass || f == kFeatSum) {
        if (first >= 2 || s.multi || s.roll) return kRefused;
        return {one, 3, rx | (f == kFeatClass ? kClass : kSum) | general_form(s)};
    }
    if (f == kFeatAov) {
        if (first >= 2 || s.receive_raw || s.roll) return kRefused;
        return {one, 3, kAov | general_form(s)};
    }
    const int m = rx | (f == kFeatMoment ? kMoment : 0);
    const int narrow = s.wide ? kWide : (s.lean ? kLean : 0);
    if (s.geom) return first >= 2 ? kRefused : ShadeForm{one, 3, m | kGeom | narrow};
    if (s.multi) return {any, 3, m | kMulti};
    if (f == kFeatMoment) return {any, 3, m | narrow};
    if (narrow == kLean && (first || waves == 3)) {
        const bool four = waves == 4 && (first == 1 || (first == 2 && !s.receive_raw));
        return {any, four ? 4 : 3, m | kLean};
    }
    if (s.wide) return {any, 3, m | kWide};
    if (first) return {any, 3, m};
    return {0, (waves >= 2 && waves <= 4) ? waves : 1, m};
}

// The wf_shade instantiations an object holds (fast: the fast-arithmetic one), stated apart from the selector above: the launcher
// instantiates exactly these and refuses any other triple, and tests/test_variant_host.py holds the selector's range to them.
constexpr bool shade_exists(bool fast, int first, int w, int v) {
    const int feature = v & (kMoment | kClass | kAov | kSum), form = v & (kWide | kLean | kMulti | kGeom);
    if (first < 0 || first > 3 || v < 0 || v != (feature | form | (v & 1))) return false;
    if (feature == kClass || feature == kSum || feature == kAov)      // general forms, both mode classes (AOV: the render modes only)
        return !fast && w == 3 && first < 2 && !(form & (kLean | kMulti)) && !(feature == kAov && (v & 1));
    if (feature != 0 && (feature != kMoment || fast || w != 3)) return false;
    switch (form) {
        case kGeom: case kGeom | kLean: case kGeom | kWide: return w == 3 && first < 2;
        case kMulti: case kWide: return w == 3;
        case kLean: return w == 3 || (w == 4 && feature == 0 && (first == 1 || (first == 2 && !(v & 1))));
        case 0: return w == 3 || (first == 0 && feature == 0 && w >= 1 && w <= 4);
        default: return false;
    }
}
// where the set lies: first < kShadeFirsts, w <= kShadeWavesMax, and every V is shade_word(i) for one i < kShadeWords (mode class x
// feature x form)
constexpr int kShadeFirsts = 4, kShadeWavesMax = 4, kShadeWords = 2 * 5 * 7;
constexpr int shade_word(int i) {
    constexpr int features[5] = {0, kMoment, kClass, kAov, kSum}, forms[7] = {0, kWide, kLean, kMulti, kGeom, kGeom | kWide, kGeom | kLean};
    return (i & 1) | features[(i >> 1) % 5] | forms[(i >> 1) / 5];
}

// ---- wf_trace<STATS, W, SHIFT, QUANT, GEOM> ----
struct TraceForm {
    bool stats;
    int w;
    bool shift, quant, geom;
    constexpr int flags() const { return (stats ? 1 : 0) | (shift ? 2 : 0) | (quant ? 4 : 0) | (geom ? 8 : 0); }      // < kTraceFlags
};
constexpr int kTraceFlags = 16, kTraceWavesMax = 6;      // where trace_exists' set lies: flags() < kTraceFlags, w <= kTraceWavesMax
constexpr TraceForm trace_form(int w, int flags) { return {(flags & 1) != 0, w, (flags & 2) != 0, (flags & 4) != 0, (flags & 8) != 0}; }

// `waves`: the budget the host asks for; shift: WF::offsets != nullptr, quant: DScene::qnodes != nullptr, geom: WF::geom_stride != 0.
// Per-render geometry versions never come with mesh offsets (a `shift` there is ignored) and have no LDS copy of the top nodes; with
// that copy five workgroups per CU are the most whose LDS fits, six with the smaller copy of the quantised nodes.
inline TraceForm trace_variant(bool stats, int waves, bool shift, bool quant, bool geom) {
    if (geom) return {stats, waves >= 5 ? 5 : 4, false, quant, true};
    return {stats, (waves >= 6 && quant) ? 6 : (waves >= 5 ? 5 : 4), shift, quant, false};
}
// the wf_trace instantiations an object holds (the same in both objects), each with and without STATS
constexpr bool trace_exists(const TraceForm &t) {
    return t.geom ? ((t.w == 4 || t.w == 5) && !t.shift) : (t.w == 4 || t.w == 5 || (t.w == 6 && t.quant));
}
}  // namespace bfv
