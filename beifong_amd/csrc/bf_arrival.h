// The arrival table behind bf_scene_set_arrival_classes (include/beifong_hip.h): the class of a path from the direction of
// its primary ray, all of its arithmetic, in plain C++ with no HIP in it, so that the device kernels (bf_path_logic.h: generate_path),
// the host entry (bf_endpoints.cpp) and a host-only test program (tests/native/arrival_check.cpp) compile the same text.
//
// The direction d is projected onto two world-space axes, u = d . axis_u and v = d . axis_v, the window [u0, u1) x [v0, v1) is cut into
// n_u x n_v bins, and a direction outside the window (a NaN included) gets class n_u n_v.  Every product and sum is an fp32 operation
// rounded on its own: no FMA, so the class is the same number wherever it is computed (capi.arrival_classes states it in numpy).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define BF_ARR_HD __host__ __device__ __forceinline__
#elif defined(__GNUC__) && !defined(__clang__)
#define BF_ARR_HD __attribute__((optimize("fp-contract=off"))) inline
#else
#define BF_ARR_HD inline
#endif
#if defined(__clang__)
#define BF_ARR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define BF_ARR_NO_CONTRACT
#endif

namespace bfa {
constexpr uint32_t kWords = 12;      // the table as the device reads it: twelve 32-bit words
// What the kernels read: the axes, each window's lower edge and scale, the bin counts.  (The upper edges are in the scales.)
struct Table {
    float axis_u[3], axis_v[3];
    float u0, su, v0, sv;
    uint32_t n_u, n_v;
};
static_assert(sizeof(Table) == kWords * 4, "the device table is twelve words");

// su = fl(fl((float) n) / fl(hi - lo)): bins per unit of the projection; computed once, on the host
BF_ARR_HD float scale(uint32_t n, float lo, float hi) {
    BF_ARR_NO_CONTRACT
    const float w = hi - lo;
    return (float) n / w;
}

// fl(fl(fl(d.x a.x) + fl(d.y a.y)) + fl(d.z a.z))
BF_ARR_HD float project(float dx, float dy, float dz, float ax, float ay, float az) {
    BF_ARR_NO_CONTRACT
    const float px = dx * ax, py = dy * ay, pz = dz * az;
    const float s = px + py;
    return s + pz;
}

// the bin coordinate tu = fl(fl(u - u0) * su)
BF_ARR_HD float coordinate(float u, float u0, float su) {
    BF_ARR_NO_CONTRACT
    const float r = u - u0;
    return r * su;
}

// the class of direction (dx, dy, dz) from the table's twelve words
BF_ARR_HD uint32_t classify(float dx, float dy, float dz, float ux, float uy, float uz, float vx, float vy, float vz, float u0, float su, float v0,
                            float sv, uint32_t n_u, uint32_t n_v) {
    const float tu = coordinate(project(dx, dy, dz, ux, uy, uz), u0, su);
    const float tv = coordinate(project(dx, dy, dz, vx, vy, vz), v0, sv);
    const bool inside = tu >= 0.f && tu < (float) n_u && tv >= 0.f && tv < (float) n_v;      // (a NaN compares false: outside)
    return inside ? (uint32_t) tv * n_u + (uint32_t) tu : n_u * n_v;
}
BF_ARR_HD uint32_t classify(const Table &t, float dx, float dy, float dz) {
    return classify(dx, dy, dz, t.axis_u[0], t.axis_u[1], t.axis_u[2], t.axis_v[0], t.axis_v[1], t.axis_v[2], t.u0, t.su, t.v0, t.sv, t.n_u, t.n_v);
}
}  // namespace bfa
