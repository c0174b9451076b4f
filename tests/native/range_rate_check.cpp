// Host-only run of bf_range_rate.h (tests/test_range_rate_host.py).  Input, per table: a line of the five fp32 bit patterns
// sensor_lin[3] r0 r1 (decimal integers), n_bins and n; then n lines of fifteen bit patterns: lin[3] ang[3] pivot[3] of the shape's
// twist, the point p[3] and the direction d[3].  Output: the bit pattern of the scale, then per line the bit pattern of the range
// rate and the class.
#include <cstdio>
#include <cstring>

#include "../../beifong_amd/csrc/bf_range_rate.h"

static float from_bits(unsigned b) {
    float f;
    std::memcpy(&f, &b, sizeof(f));
    return f;
}
static unsigned to_bits(float f) {
    unsigned b;
    std::memcpy(&b, &f, sizeof(b));
    return b;
}

int main() {
    unsigned w[5], n_bins, n;
    for (;;) {
        int got = 0;
        for (int i = 0; i < 5; ++i) got += std::scanf("%u", &w[i]) == 1;
        if (got == 0) return 0;
        if (got != 5 || std::scanf("%u %u", &n_bins, &n) != 2) return 1;
        bfr::Header h = {};
        for (int i = 0; i < 3; ++i) h.sensor_lin[i] = from_bits(w[i]);
        h.r0 = from_bits(w[3]);
        h.sr = bfa::scale(n_bins, h.r0, from_bits(w[4]));
        h.n_bins = n_bins;
        std::printf("%u\n", to_bits(h.sr));
        for (unsigned i = 0; i < n; ++i) {
            unsigned v[15];
            for (int j = 0; j < 15; ++j)
                if (std::scanf("%u", &v[j]) != 1) return 1;
            bfr::Row r = {};
            for (int j = 0; j < 3; ++j) r.lin[j] = from_bits(v[j]), r.ang[j] = from_bits(v[3 + j]), r.pivot[j] = from_bits(v[6 + j]);
            const float p[3] = {from_bits(v[9]), from_bits(v[10]), from_bits(v[11])}, d[3] = {from_bits(v[12]), from_bits(v[13]), from_bits(v[14])};
            const float rr = bfr::rate(p[0], p[1], p[2], d[0], d[1], d[2], r.lin[0], r.lin[1], r.lin[2], r.ang[0], r.ang[1], r.ang[2], r.pivot[0],
                                       r.pivot[1], r.pivot[2], h.sensor_lin[0], h.sensor_lin[1], h.sensor_lin[2]);
            std::printf("%u %u\n", to_bits(rr), bfr::classify(h, r, p[0], p[1], p[2], d[0], d[1], d[2]));
        }
    }
}
