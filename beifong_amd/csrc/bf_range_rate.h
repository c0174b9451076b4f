// The range-rate table behind bf_scene_set_range_rate_classes (include/beifong_hip.h): the class of a path from the range
// rate of its first intersection seen along its primary ray, all of its arithmetic, in plain C++ with no HIP in it, so that the device
// kernels (bf_path_logic.h: shade_vertex), the host entry (bf_endpoints.cpp) and a host-only test program
// (tests/native/range_rate_check.cpp) compile the same text.
//
// Shape k moves rigidly: its point p has velocity lin_k + ang_k x (p - pivot_k); the radar moves with sensor_lin.  The range rate is the
// relative velocity projected on the primary ray's direction d (positive: an opening range), the window [r0, r1) is cut into n_bins bins,
// and a rate outside it (a NaN included) gets class n_bins.  Every product, sum and difference is an fp32 operation rounded on its own:
// no FMA (contraction is switched off here, in the text), so the class is the same number wherever it is computed
// (capi.range_rate_classes states it in numpy).
#pragma once
#include <stdint.h>

#include "bf_arrival.h"

namespace bfr {
constexpr uint32_t kHeaderWords = 8;      // the table as the device reads it: a header of eight 32-bit words ...
constexpr uint32_t kRowWords = 12;        // ... and twelve per shape: three 16-byte loads, each row 16-byte aligned behind the header
// What the kernels read ahead of the rows: the radar's velocity, the window's lower edge and scale, the bin count.
struct Header {
    float sensor_lin[3];
    float r0, sr;
    uint32_t n_bins;
    uint32_t pad[2];      // the address of the velocity rows, low and high half (bf_velocity.h); 0 while no shape has a velocity mode
};
// The twist of one shape, each vector in a 16-byte word of its own.
struct Row {
    float lin[3], pad0;      // pad0: the bits of the shape's BF_VELOCITY_* mode (bf_velocity.h); 0: the twist alone
    float ang[3], pad1;
    float pivot[3], pad2;
};
static_assert(sizeof(Header) == kHeaderWords * 4 && sizeof(Row) == kRowWords * 4 && sizeof(Header) % 16 == 0, "the device table: 8 + 12 n_shapes words");
constexpr uint64_t table_words(uint32_t n_shapes) { return kHeaderWords + (uint64_t) kRowWords * n_shapes; }

// one component of ang x q: fl(fl(a q') - fl(a' q))
BF_ARR_HD float cross_component(float a, float qn, float an, float q) {
    BF_ARR_NO_CONTRACT
    const float l = a * qn, r = an * q;
    return l - r;
}
// one component of the relative velocity: fl(fl(lin + c) - sensor_lin)
BF_ARR_HD float relative(float lin, float c, float sensor_lin) {
    BF_ARR_NO_CONTRACT
    const float v = lin + c;
    return v - sensor_lin;
}
BF_ARR_HD float lever(float p, float pivot) {
    BF_ARR_NO_CONTRACT
    return p - pivot;
}

// rr: the velocity of point p of a shape with twist (lin, ang, pivot), relative to the radar, along d
BF_ARR_HD float rate(float px, float py, float pz, float dx, float dy, float dz, float lx, float ly, float lz, float ax, float ay, float az, float ox,
                     float oy, float oz, float sx, float sy, float sz) {
    const float qx = lever(px, ox), qy = lever(py, oy), qz = lever(pz, oz);
    const float cx = cross_component(ay, qz, az, qy), cy = cross_component(az, qx, ax, qz), cz = cross_component(ax, qy, ay, qx);
    return bfa::project(dx, dy, dz, relative(lx, cx, sx), relative(ly, cy, sy), relative(lz, cz, sz));
}

// the class of range rate rr: its bin, or n_bins outside the window (a NaN compares false: outside; -0 >= 0: inside)
BF_ARR_HD uint32_t classify(float rr, float r0, float sr, uint32_t n_bins) {
    const float t = bfa::coordinate(rr, r0, sr);
    return (t >= 0.f && t < (float) n_bins) ? (uint32_t) t : n_bins;
}
BF_ARR_HD uint32_t classify(const Header &h, const Row &w, float px, float py, float pz, float dx, float dy, float dz) {
    return classify(rate(px, py, pz, dx, dy, dz, w.lin[0], w.lin[1], w.lin[2], w.ang[0], w.ang[1], w.ang[2], w.pivot[0], w.pivot[1], w.pivot[2],
                         h.sensor_lin[0], h.sensor_lin[1], h.sensor_lin[2]),
                    h.r0, h.sr, h.n_bins);
}
}  // namespace bfr
