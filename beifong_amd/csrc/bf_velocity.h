// Per-vertex velocities under the range-rate table (include/beifong_hip.h: bf_scene_set_velocity_mode): the velocity of a
// triangle's corner from two rendered positions, its interpolation at a hit, and the range rate of a point that carries such a
// velocity on top of its shape's twist, all of the arithmetic, in plain C++ with no HIP in it, so that the device kernels
// (bf_geom.hip: bf_velocity_diff_kernel; bf_path_logic.h: shade_vertex), and a host-only test program (tests/native/velocity_check.cpp)
// compile the same text.
//
// A mesh shape is in one of three modes: its points move with the shape's twist alone (0, bf_range_rate.h as it stands), or with
// the twist plus a velocity interpolated from the three corners of the triangle hit, which the caller has given per vertex (1) or
// which is the difference of two rendered positions over a time step (2).  Every product, sum, difference and quotient is an fp32
// operation rounded on its own: no FMA (contraction is switched off here, in the text), so the class is the same number wherever it
// is computed (capi.interpolate_velocity, capi.corner_velocities and capi.range_rate_classes state it in numpy).
#pragma once
#include <stdint.h>

#include "bf_range_rate.h"

namespace bfvel {
constexpr uint32_t kTwist = 0, kVertex = 1, kDifference = 2;      // BF_VELOCITY_*
constexpr uint32_t kRowsPerSlot = 3;      // the velocity rows: one 16-byte row per corner of a triangle slot, in face order

// one component of a corner's velocity from its rendered positions: fl(fl(next - prev) / dt), IEEE division
BF_ARR_HD float corner(float prev, float next, float dt) {
    BF_ARR_NO_CONTRACT
    const float d = next - prev;
    return d / dt;
}
// the first barycentric of a hit at (u, v): fl(fl(1 - u) - v)
BF_ARR_HD float b0(float u, float v) {
    BF_ARR_NO_CONTRACT
    const float a = 1.f - u;
    return a - v;
}
// one component of the velocity at the hit: fl(fl(fl(b0 v0) + fl(u v1)) + fl(v v2))
BF_ARR_HD float interpolate(float w0, float u, float v, float v0, float v1, float v2) {
    BF_ARR_NO_CONTRACT
    const float a = w0 * v0, b = u * v1, c = v * v2;
    const float s = a + b;
    return s + c;
}
// one component of the relative velocity: fl(fl(fl(lin + c) + U) - sensor_lin)
BF_ARR_HD float relative(float lin, float c, float U, float sensor_lin) {
    BF_ARR_NO_CONTRACT
    const float t = lin + c;
    const float w = t + U;
    return w - sensor_lin;
}

// rr: bfr::rate for a point that moves with U = (Ux, Uy, Uz) on top of its shape's twist
BF_ARR_HD float rate(float px, float py, float pz, float dx, float dy, float dz, float lx, float ly, float lz, float ax, float ay, float az, float ox,
                     float oy, float oz, float sx, float sy, float sz, float Ux, float Uy, float Uz) {
    const float qx = bfr::lever(px, ox), qy = bfr::lever(py, oy), qz = bfr::lever(pz, oz);
    const float cx = bfr::cross_component(ay, qz, az, qy), cy = bfr::cross_component(az, qx, ax, qz), cz = bfr::cross_component(ax, qy, ay, qx);
    return bfa::project(dx, dy, dz, relative(lx, cx, Ux, sx), relative(ly, cy, Uy, sy), relative(lz, cz, Uz, sz));
}
}  // namespace bfvel
