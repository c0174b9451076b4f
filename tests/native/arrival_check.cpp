// Host-only run of bf_arrival.h (tests/test_arrival_host.py).  Input, per table: a line of the ten fp32 bit patterns axis_u[3]
// axis_v[3] u0 u1 v0 v1 (decimal integers), n_u, n_v and n; then n lines "x y z", the bit patterns of a direction.  Output: the
// bit patterns of the two scales on one line, then the class of every direction, one per line.
#include <cstdio>
#include <cstring>

#include "../../beifong_amd/csrc/bf_arrival.h"

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
    unsigned w[10], n_u, n_v, n;
    for (;;) {
        int got = 0;
        for (int i = 0; i < 10; ++i) got += std::scanf("%u", &w[i]) == 1;
        if (got == 0) return 0;
        if (got != 10 || std::scanf("%u %u %u", &n_u, &n_v, &n) != 3) return 1;
        bfa::Table t;
        for (int i = 0; i < 3; ++i) t.axis_u[i] = from_bits(w[i]), t.axis_v[i] = from_bits(w[3 + i]);
        t.u0 = from_bits(w[6]);
        t.v0 = from_bits(w[8]);
        t.su = bfa::scale(n_u, t.u0, from_bits(w[7]));
        t.sv = bfa::scale(n_v, t.v0, from_bits(w[9]));
        t.n_u = n_u;
        t.n_v = n_v;
        std::printf("%u %u\n", to_bits(t.su), to_bits(t.sv));
        for (unsigned i = 0; i < n; ++i) {
            unsigned x, y, z;
            if (std::scanf("%u %u %u", &x, &y, &z) != 3) return 1;
            std::printf("%u\n", bfa::classify(t, from_bits(x), from_bits(y), from_bits(z)));
        }
    }
}
