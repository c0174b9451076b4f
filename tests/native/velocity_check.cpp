// Host-only run of bf_velocity.h (tests/test_velocity_host.py).  Input: n, then n lines of 33 fp32 bit patterns (decimal integers):
// the corner positions before prev[3][3] and after next[3][3] in face order, dt, the barycentrics u v, lin[3] ang[3] pivot[3] of the
// shape's twist and sensor_lin[3]; then a line r0 r1 (bit patterns) and n_bins.  The point and the direction of the rate are taken
// from the same numbers, p = (next[0][0], next[1][1], next[2][2]) and d = (ang.x, lin.y, pivot.z): any finite vectors do.  Output
// per line: the nine bit patterns of the corner velocities, the three of the interpolated velocity, the bit pattern of the range
// rate and the class.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../beifong_amd/csrc/bf_velocity.h"

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
    unsigned n = 0;
    if (std::scanf("%u", &n) != 1) return 1;
    std::vector<float> in((size_t) n * 33);
    for (size_t i = 0; i < in.size(); ++i) {
        unsigned b;
        if (std::scanf("%u", &b) != 1) return 1;
        in[i] = from_bits(b);
    }
    unsigned r0b, r1b, n_bins;
    if (std::scanf("%u %u %u", &r0b, &r1b, &n_bins) != 3) return 1;
    const float r0 = from_bits(r0b), sr = bfa::scale(n_bins, r0, from_bits(r1b));
    for (unsigned i = 0; i < n; ++i) {
        const float *v = &in[(size_t) i * 33];
        const float *prev = v, *next = v + 9, dt = v[18], u = v[19], w = v[20], *lin = v + 21, *ang = v + 24, *piv = v + 27, *sl = v + 30;
        float V[9], U[3];
        for (int j = 0; j < 9; ++j) V[j] = bfvel::corner(prev[j], next[j], dt);
        const float w0 = bfvel::b0(u, w);
        for (int c = 0; c < 3; ++c) U[c] = bfvel::interpolate(w0, u, w, V[c], V[3 + c], V[6 + c]);
        const float p[3] = {next[0], next[4], next[8]}, d[3] = {ang[0], lin[1], piv[2]};
        const float rr = bfvel::rate(p[0], p[1], p[2], d[0], d[1], d[2], lin[0], lin[1], lin[2], ang[0], ang[1], ang[2], piv[0], piv[1], piv[2], sl[0],
                                   sl[1], sl[2], U[0], U[1], U[2]);
        for (int j = 0; j < 9; ++j) std::printf("%u ", to_bits(V[j]));
        std::printf("%u %u %u %u %u\n", to_bits(U[0]), to_bits(U[1]), to_bits(U[2]), to_bits(rr), bfr::classify(rr, r0, sr, n_bins));
    }
    return 0;
}
