// Every host-callable launcher (bfk_*) of bf_kernels.hip, bf_wavefront.hip, bf_geom.hip and bf_query.hip, declared once.  The .hip
// file that defines a launcher includes this header and so do the .cpp files that call it: the launchers have C linkage, so a
// parameter list that differs between the two sides would still link; seen together it is the compile error "conflicting types".
// (bf_build.h and bf_converge.h do the same for bf_build.hip and bf_converge.hip.)  Which instantiation a render launcher runs is
// bf_variant.h, which takes the launch as bfk_launch_shape below describes it.
#pragma once
#include <hip/hip_runtime.h>

#include "bf_device.h"
#include "bf_variant.h"
#include "bf_wavefront.h"

// The launchers a render goes through, once per family of kernels: the exact build (no suffix), the fast-arithmetic build (_fast,
// BF_FLAG_FAST: bf_ns.h) and, in the exact build only, the second-moment (_moment, BF_FLAG_MOMENT; bf_device.h: kMoment), class
// (_class, BF_FLAG_CLASSES; kClass), AOV (_aov, BF_FLAG_AOV; kAov) and exact-sum (_sum, BF_FLAG_EXACT_SUM; kSum) variants, which share
// the exact wf_trace.
#define BF_RENDER_LAUNCHERS(sfx)                                                                                                                \
    extern "C" hipError_t bfk_launch_render##sfx(const bfd::DScene *sc, const bfd::DLaunch *lp, float *g_hist, bf_path_record *records,         \
                                                 unsigned long long *counters, int stats, unsigned grid, size_t lds_bytes, hipStream_t stream); \
    extern "C" hipError_t bfk_wf_shade##sfx(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it, int first,           \
                                            float *g_hist, bf_path_record *records, unsigned grid, size_t lds_bytes, hipStream_t stream,       \
                                            int waves);                                                                                         \
    extern "C" hipError_t bfk_launch_tail##sfx(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it, uint32_t n_slots, \
                                               float *g_hist, bf_path_record *records, int stats, size_t lds_bytes, hipStream_t stream,        \
                                               int tail_waves, unsigned spread, unsigned block_cap);
#define BF_TRACE_LAUNCHER(sfx) \
    extern "C" hipError_t bfk_wf_trace##sfx(const bfd::DScene *sc, const bfd::WF *wf, uint32_t it, int stats, unsigned grid, hipStream_t stream, int waves);

// the shape of a launch as bf_variant.h's selectors take it (tail_waves: the tail's launchers alone)
static inline bfv::Shape bfk_launch_shape(const bfd::DLaunch &lp, int tail_waves = 0) {
    return {lp.geom_stride != 0, lp.wide != 0, lp.lean != 0, lp.multi != 0, lp.roll != 0, lp.mode == BF_MODE_RECEIVE_RAW, tail_waves == 2};
}

#if BF_FAST
// A fast device file: bfd::DScene, DLaunch and WF are bfd::fast:: types here, so it sees the family it defines and nothing else (the
// other families' prototypes would name the same C functions with other parameter types)
BF_RENDER_LAUNCHERS(_fast)
BF_TRACE_LAUNCHER(_fast)
#else
// An exact device file (which defines the first five families) or a host file (which calls all six)
BF_RENDER_LAUNCHERS()
BF_RENDER_LAUNCHERS(_moment)
BF_RENDER_LAUNCHERS(_class)
BF_RENDER_LAUNCHERS(_aov)
BF_RENDER_LAUNCHERS(_sum)
BF_RENDER_LAUNCHERS(_fast)
BF_TRACE_LAUNCHER()
BF_TRACE_LAUNCHER(_fast)

// bf_kernels.hip: one descriptor of a rolling sequence's ring (bf_render.cpp)
extern "C" hipError_t bfk_roll_set(bfd::DRoll *ring, float4 *offsets, uint32_t idx, const bfd::DRoll *d, const float *offset3, hipStream_t stream);

// bf_geom.hip: the launchers that move geometry (bf_mesh.cpp, bf_pose.cpp)
extern "C" hipError_t bfk_launch_translate(const float4 *tris0, float4 *tris, uint32_t n_tri_rows, const float4 *nodes0,
                                           float4 *nodes, float4 *qnodes, uint32_t n_nodes, const float4 *wnodes0, float4 *wnodes,
                                           uint32_t n_wchildren, const float *d, hipStream_t stream);
extern "C" hipError_t bfk_launch_deform_tris(const uint4 *corners, const bfd::DDeformSrc *src, const float4 *tris0, float4 *tris, const float4 *nrm0,
                                             float4 *nrm, uint32_t n_tris, const float *xf, uint32_t n_versions, uint64_t vstride,
                                             uint32_t xf_stride, float bound, uint32_t *bad, hipStream_t stream);
// the velocity rows (bf_velocity.h): differenced from two sets of triangle rows, and gathered from an explicit per-vertex field
extern "C" hipError_t bfk_launch_velocity_diff(const float4 *prev, const float4 *next, float4 *vel, const float4 *own, uint32_t n_tris,
                                               const float2 *modes, uint32_t n_versions, uint64_t vstride, uint32_t tail_prev, uint32_t tail_next,
                                               hipStream_t stream);
extern "C" hipError_t bfk_launch_velocity_gather(const uint4 *corners, const float4 *tris, const float *field, uint32_t shape, float4 *vel,
                                                 uint32_t n_tris, hipStream_t stream);
extern "C" hipError_t bfk_launch_refit(const float4 *tris, const float4 *nodes0, float4 *nodes, float4 *qnodes, uint32_t n_nodes, const uint32_t *lvl4,
                                       const uint32_t *lvl4_off, uint32_t n_lvl4, float4 *ubox4, const float4 *wnodes0, float4 *wnodes,
                                       const uint32_t *lvl16, const uint32_t *lvl16_off, uint32_t n_lvl16, float4 *ubox16, float abs_pad,
                                       uint32_t n_versions, uint64_t vstride, hipStream_t stream);
extern "C" hipError_t bfk_launch_rigid(const float4 *tris0, float4 *tris, const float4 *nrm0, float4 *nrm, uint32_t n_tris,
                                       const float *xf, const float4 *nodes0, float4 *nodes, float4 *qnodes, uint32_t n_nodes, const uint32_t *lvl4,
                                       const uint32_t *lvl4_off, uint32_t n_lvl4, float4 *ubox4, const float4 *wnodes0, float4 *wnodes, const uint32_t *lvl16,
                                       const uint32_t *lvl16_off, uint32_t n_lvl16, float4 *ubox16, float abs_pad, uint32_t n_versions,
                                       uint64_t vstride, uint32_t xf_stride, hipStream_t stream);
extern "C" hipError_t bfk_launch_skin_vertices(const float *rest_pos, const float *rest_nrm, const uint4 *index, const float4 *weight, uint32_t nv,
                                               const float *bones, uint32_t n_bones, float *pos, float *nrm, uint32_t n_versions,
                                               hipStream_t stream);
extern "C" hipError_t bfk_launch_morph_vertices(const float *rest_pos, const float *rest_nrm, const float *dpos, const float *dnrm, uint32_t nv,
                                                uint32_t n_targets, const float *wts, const uint4 *index, const float4 *weight,
                                                const float *bones, uint32_t n_bones, int dq, float *pos, float *nrm, uint32_t n_versions,
                                                hipStream_t stream);
extern "C" hipError_t bfk_launch_skin_vertices_dq(const float *rest_pos, const float *rest_nrm, const uint4 *index, const float4 *weight,
                                                  uint32_t nv, const float *bones, uint32_t n_bones, float *pos, float *nrm,
                                                  uint32_t n_versions, hipStream_t stream);
extern "C" hipError_t bfk_launch_vertex_normals(const uint32_t *offset, const uint4 *entries, uint32_t nv, const float *pos, float *nrm,
                                                uint32_t n_versions, hipStream_t stream);
extern "C" void bfk_host_vertex_normals(uint32_t nv, const float *pos, uint32_t nf, const uint32_t *idx, float *out);

// bf_query.hip: batch ray queries, the plugin-level queries (op 0 BSDF eval + pdf, 1 BSDF sample, 2 emitter sample_direction, 3 sensor
// sample_ray), the microfacet and elementary-function probes, the gather probe, and the engine's cosine on the host (bf_api.cpp,
// bf_endpoints.cpp)
extern "C" hipError_t bfk_launch_trace(const bfd::DScene *sc, uint64_t n, const float *rays, int any_hit, float *out_t,
                                       uint32_t *out_prim, uint32_t *out_shape, float *out_uv, uint8_t *out_hit,
                                       float *out_si, hipStream_t stream);
extern "C" hipError_t bfk_launch_query(int op, const bfd::DScene *sc, uint64_t n, const uint32_t *materials, uint32_t emitter,
                                       const float *in, float *out, hipStream_t stream);
extern "C" hipError_t bfk_launch_microfacet(int op, uint32_t type, float alpha_u, float alpha_v, uint32_t sample_visible, uint64_t n,
                                            const float *in, float *out, hipStream_t stream);
extern "C" hipError_t bfk_launch_elementary(int op, uint64_t n, const float *x, float *y);
extern "C" hipError_t bfk_gather_probe(int mode, const float4 *table, uint32_t n_rows, float4 *out, hipStream_t stream);
extern "C" float bfk_host_cos(float x);

// bf_sum.hip (BF_FLAG_EXACT_SUM): the limb cells of a launch into its histogram, hist[i] = fl(hist[i] + cell i) for every cell that
// received an addend; and the probe behind bf_exact_sum: n (cell, value) pairs into n_cells limb cells (zeroed by the caller), in LDS
// per workgroup first with in_lds (n_cells * 72 bytes of dynamic LDS)
extern "C" hipError_t bfk_sum_resolve(const void *limbs, float *hist, uint32_t n_cells, hipStream_t stream);
extern "C" hipError_t bfk_sum_probe(uint64_t n, const uint32_t *cell, const float *value, uint32_t n_cells, int in_lds, void *limbs,
                                    unsigned grid, hipStream_t stream);
#endif

#undef BF_RENDER_LAUNCHERS
#undef BF_TRACE_LAUNCHER
