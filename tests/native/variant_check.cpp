// Host-only walk over bf_variant.h (tests/test_variant_host.py): one line per combination, led by the kind of line,
//   0 | 1  feature geom wide lean multi two roll raw              word        render_variant (0) and tail_variant (1); -1: refused
//   2      feature fast first waves geom wide lean multi two roll raw   FIRST W V     shade_variant; FIRST -1: refused
//   3      stats waves shift quant geom                           STATS W SHIFT QUANT GEOM      trace_variant
//   4      fast first w v                                                     a triple of shade_exists
//   5      stats w shift quant geom                                           a tuple of trace_exists
// The stated sets are searched well beyond where they lie, and must lie where the launchers look for them.
#include <cstdio>

#include "../../beifong_amd/csrc/bf_variant.h"

static bfv::Shape shape(int bits) {
    bfv::Shape s;
    s.geom = bits & 1, s.wide = bits & 2, s.lean = bits & 4, s.multi = bits & 8, s.two = bits & 16, s.roll = bits & 32;
    s.receive_raw = bits & 64;
    return s;
}

int main() {
    for (int kind = 0; kind < 2; ++kind)
        for (int f = 0; f < 5; ++f)
            for (int bits = 0; bits < 128; ++bits) {
                const bfv::Shape s = shape(bits);
                const int w = kind ? bfv::tail_variant((bfv::Feature) f, s) : bfv::render_variant((bfv::Feature) f, s);
                std::printf("%d %d %d %d %d %d %d %d %d %d\n", kind, f, (int) s.geom, (int) s.wide, (int) s.lean, (int) s.multi, (int) s.two,
                            (int) s.roll, (int) s.receive_raw, w);
            }
    for (int f = 0; f < 5; ++f)
        for (int fast = 0; fast < 2; ++fast)
            for (int first = 0; first < 4; ++first)
                for (int waves = 0; waves < 6; ++waves)
                    for (int bits = 0; bits < 128; ++bits) {
                        const bfv::Shape s = shape(bits);
                        const bfv::ShadeForm r = bfv::shade_variant((bfv::Feature) f, fast != 0, s, first, waves);
                        std::printf("2 %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", f, fast, first, waves, (int) s.geom, (int) s.wide, (int) s.lean,
                                    (int) s.multi, (int) s.two, (int) s.roll, (int) s.receive_raw, r.first, r.w, r.v);
                    }
    for (int bits = 0; bits < 16; ++bits)
        for (int waves = 3; waves < 8; ++waves) {
            const bfv::TraceForm t = bfv::trace_variant(bits & 1, waves, bits & 2, bits & 4, bits & 8);
            std::printf("3 %d %d %d %d %d %d %d %d %d %d\n", bits & 1, waves, (bits >> 1) & 1, (bits >> 2) & 1, (bits >> 3) & 1, (int) t.stats, t.w,
                        (int) t.shift, (int) t.quant, (int) t.geom);
            if (bfv::trace_form(t.w, t.flags()).flags() != t.flags() || t.flags() >= bfv::kTraceFlags) return 1;
        }
    for (int fast = 0; fast < 2; ++fast)
        for (int first = -1; first < 6; ++first)
            for (int w = -1; w < 10; ++w)
                for (int v = -1; v < 2048; ++v) {
                    if (!bfv::shade_exists(fast != 0, first, w, v)) continue;
                    std::printf("4 %d %d %d %d\n", fast, first, w, v);
                    bool listed = false;
                    for (int i = 0; i < bfv::kShadeWords; ++i) listed = listed || bfv::shade_word(i) == v;
                    if (!listed || first >= bfv::kShadeFirsts || w > bfv::kShadeWavesMax) return 1;      // outside the sequences wf_shade_launch folds over
                }
    for (int flags = 0; flags < bfv::kTraceFlags; ++flags)
        for (int w = -1; w < 12; ++w) {
            const bfv::TraceForm t = bfv::trace_form(w, flags);
            if (!bfv::trace_exists(t)) continue;
            std::printf("5 %d %d %d %d %d\n", (int) t.stats, t.w, (int) t.shift, (int) t.quant, (int) t.geom);
            if (w < 0 || w > bfv::kTraceWavesMax) return 1;
        }
    return 0;
}
