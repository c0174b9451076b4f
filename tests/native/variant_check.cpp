// Host-only walk over bf_variant.h (tests/test_variant_host.py): one line per combination of kind, feature and launch shape,
//   kind feature geom wide lean multi two roll raw word
// with kind 0 = render, 1 = tail and word = -1 for a refused launch.
#include <cstdio>

#include "../../beifong_amd/csrc/bf_variant.h"

int main() {
    for (int kind = 0; kind < 2; ++kind)
        for (int f = 0; f < 4; ++f)
            for (int bits = 0; bits < 128; ++bits) {
                bfv::Shape s;
                s.geom = bits & 1, s.wide = bits & 2, s.lean = bits & 4, s.multi = bits & 8, s.two = bits & 16, s.roll = bits & 32;
                s.receive_raw = bits & 64;
                const int w = kind ? bfv::tail_variant((bfv::Feature) f, s) : bfv::render_variant((bfv::Feature) f, s);
                std::printf("%d %d %d %d %d %d %d %d %d %d\n", kind, f, (int) s.geom, (int) s.wide, (int) s.lean, (int) s.multi, (int) s.two,
                            (int) s.roll, (int) s.receive_raw, w);
            }
    return 0;
}
