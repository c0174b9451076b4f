// What a path carries from one kernel visit to the next, shared verbatim by the wavefront kernels (bf_wavefront.hip) and the
// megakernel / tail kernel (bf_kernels.hip): the flag bits, PathState and its rows in the wavefront pool (bf_wavefront.h: WF),
// and the scene and mesh shift the path's render sees (path_scene, path_shift).  The reference keeps all of this in the locals of
// one call of SamplingIntegrator::render_sample / receive_sample (integrator.cpp:259-283, 1538-1572) and of the integrator's
// sample() loop (path.cpp:100-226 and its pathlength / pathtime / pathtimefrequency variants); ray.time and ray.phase are
// Ray::update_state's (ray.h:89-93).
#pragma once
#include "bf_device_core.h"
#include "bf_wavefront.h"

BF_NS_BEGIN

constexpr uint32_t kFlagValid = 1u << 24, kFlagFilmOk = 1u << 25, kFlagTermPending = 1u << 26, kDepthMask = 0xffffffu;
// multi-pixel films: the sample landed in the left / upper neighbour of the pixel it was drawn in (ImageBlock::put)
constexpr uint32_t kFlagFilmLeft = 1u << 27, kFlagFilmUp = 1u << 28;
// the stored state lacks the term of the NEE shadow ray wf_shade handed to wf_trace with it: load_state adds it (stored states only)
constexpr uint32_t kFlagShadowPending = 1u << 29;

struct PathState {
    V3 ro, rd;
    float rmint, rmaxt;
    float throughput, eta, emission_weight, result;
    float aux, bs_pdf;
    V3 prev_p;
    uint32_t flags;      // depth | kFlag*
    uint32_t n_rays;
    Rng rng;
    uint64_t path_i;     // index within the launch; batched launches: global index over all renders (render * batch_paths + local)
    uint32_t render;     // batched launches: which render of the batch this path belongs to (0 otherwise)
    // gen-3 (receive) only
    float time;          // ray.time: retarded time carried along the path (ray.h:89-93)
    float t_rx;          // sampled receive time (integrator.cpp:1556-1561)
    float lambda0;       // ray.wavelengths[0] in nm
    float phase;         // ray.phase of the working ray: last traced segment only (ray.h:89-93, interaction.h:61-64)
    float dlambda;       // BF_FLAG_DOPPLER: what the Doppler hook has added to the caller's ray.wavelengths[0] (nm)
    uint32_t cls;        // kClass: shape_class of the path's first intersection, miss_class until then; under an arrival table the bin of the
                         // primary ray's direction, from generation on; under a range-rate table the bin of the first intersection's
                         // range rate (the other variants never touch it: no register)
};

// `classed`: a compile-time constant at every call site ((V & kClass) != 0).  `hq`: the slot's hit row — the same 64-byte record as
// the ray, fetched with the state (the caller reads it unless the path's film write is pending).
// Two round trips: the state rows and the hit; then, only for a state stored with kFlagShadowPending, the row that holds the
// shadow request's contribution and wf_trace's answer — the round trip the hit used to take, and no third cache line for the
// states that wait for no shadow ray.
BF_DEV void load_state(const WF &wf, uint32_t i, bool receive, PathState &s, float4 &hq, bool classed = false) {
    float4 r0 = wf.ray0(i), r1 = wf.ray1(i), a = wf.sa(i), bb = wf.sb(i);
    uint4 d = wf.sd(i);
    hq = wf.hit(i);
    s.ro = mk(r0.x, r0.y, r0.z);
    s.rmint = r0.w;
    s.rd = mk(r1.x, r1.y, r1.z);
    s.rmaxt = r1.w;
    s.throughput = a.x;
    s.eta = a.y;
    s.emission_weight = a.z;
    s.result = a.w;
    s.aux = bb.x;
    s.bs_pdf = bb.y;
    s.prev_p = s.ro;             // the previous vertex IS the origin of the ray in flight (spawn_ray, interaction.h:61-64)
    s.flags = __float_as_uint(bb.z);
    s.n_rays = __float_as_uint(bb.w);
    s.rng.state = ((uint64_t) d.y << 32) | d.x;
    s.path_i = ((uint64_t) d.w << 32) | d.z;
    s.time = s.t_rx = s.lambda0 = s.phase = 0.f;
    s.render = wf.has_render ? wf.render(i) : 0u;
    s.dlambda = wf.has_dop ? wf.dop(i) : 0.f;
    if (classed) s.cls = wf.cls(i);
    if (receive) {
        float4 e = wf.se(i);
        s.time = e.x;
        s.t_rx = e.y;
        s.lambda0 = e.z;
        s.phase = e.w;
    }
    if (s.flags & kFlagShadowPending) {
        // wf_trace has answered the shadow ray stored with this state (q.z: occluded).  Scene::sample_emitter_direction zeroes
        // the VALUE of an occluded sample (scene.cpp:220-224) and the integrator still adds mis * throughput * bsdf * 0: a
        // NaN / inf BSDF value survives that product.  c * 0 is that term (+-0 for every finite c).  Applied before anything
        // else touches the state: the same fp32 add wf_shade does for a ray it answers itself.
        const float4 q = wf.sh23(i);
        const bool occ = __float_as_uint(q.z) != 0u;
        s.result += occ ? q.x * 0.f : q.x;
        if (receive && wf.iq) s.phase += occ ? q.y * 0.f : q.y;      // BF_MODE_RECEIVE_IQ: the imaginary accumulator
        s.flags &= ~kFlagShadowPending;
    }
}
BF_DEV void store_state(const WF &wf, uint32_t j, bool receive, const PathState &s, bool classed = false) {
    wf.ray0(j) = make_float4(s.ro.x, s.ro.y, s.ro.z, s.rmint);
    wf.ray1(j) = make_float4(s.rd.x, s.rd.y, s.rd.z, s.rmaxt);
    wf.sa(j) = make_float4(s.throughput, s.eta, s.emission_weight, s.result);
    wf.sb(j) = make_float4(s.aux, s.bs_pdf, __uint_as_float(s.flags), __uint_as_float(s.n_rays));
    wf.sd(j) = make_uint4((uint32_t) s.rng.state, (uint32_t) (s.rng.state >> 32), (uint32_t) s.path_i,
                          (uint32_t) (s.path_i >> 32));
    if (receive) wf.se(j) = make_float4(s.time, s.t_rx, s.lambda0, s.phase);
    if (wf.has_render) wf.render(j) = s.render;
    if (wf.has_dop) wf.dop(j) = s.dlambda;
    if (classed) wf.cls(j) = s.cls;
}
// The scene a path of render `render` sees.  Plain launches and sequences whose endpoints stand still: the launch's own
// (wave-uniform: the tables are read through the scalar cache).  kMulti: the table pointers and physics of the path's render out
// of the descriptor ring — a per-lane record, so everything read through them is a vector load.  kGeom: the geometry arrays of
// the path's render (DLaunch::geom_stride rows per render; the topology — root, stack bounds, spill columns — is shared).
template <int V> BF_DEV DScene path_scene(const DScene &sc, const DLaunch &lp, uint32_t render) {
    if (!(V & (kMulti | kGeom))) return sc;
    DScene r = sc;
    if (V & kMulti) {
        const BF_CAS DRoll &e = as_const(lp.roll)[render & (kRollRing - 1u)];
        r.rects = e.rects;
        r.shapes = e.shapes;
        r.emitters = e.emitters;
        r.materials = e.materials;
        r.sensor = e.sensor;
        r.c = e.c;
        r.lambda_min = e.lambda_min;
        r.lambda_max = e.lambda_max;
        r.tab_on = 0u;                 // (the workgroup's LDS copies hold one version)
    }
    if (V & kGeom) geom_version(r, (uint64_t) render * lp.geom_stride);
    return r;
}
// the mesh shift of the path's render (batched launches with moving meshes; off otherwise)
BF_DEV Shift path_shift(const DLaunch &lp, uint32_t render) { return make_shift(lp.batch_offsets, render, lp.box_slack); }

BF_NS_END  // namespace bfd
