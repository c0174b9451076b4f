// The integrator's per-path logic, shared verbatim by the wavefront shade
// kernel (bf_wavefront.hip) and the megakernel / tail kernel (bf_kernels.hip):
//
//   generate_path : SamplingIntegrator::render_sample / receive_sample head
//                   (integrator.cpp:259-283, 1538-1572) — sampler draws and the
//                   sensor / receiver ray
//   shade_vertex  : one iteration of PathIntegrator::sample (path.cpp:121-209),
//                   PathLengthIntegrator (pathlength.cpp), PathTimeIntegrator
//                   (pathtime.cpp) or PathTimeFrequencyIntegrator
//                   (pathtimefrequency.cpp:154-447), given the closest hit of the
//                   path's current ray
//   aov_store ... : AOVIntegrator's first-intersection values (aov.cpp:170-251),
//                   kept in the slot's side rows until the sample is put
//
// The NEE contribution is computed BEFORE its shadow ray is traced and handed
// to the caller (ShadowReq), which adds it to PathState::result iff the ray is
// unoccluded — the same value the reference adds (scene.cpp:220-224 zeroes the
// emitter value of an occluded sample).
//
// The state a path carries is in bf_path_state.h, the transmitter / receiver
// arithmetic in bf_endpoint_logic.h; what becomes of a finished path's sample
// is bf_film.h's, which builds on this file.
#pragma once
#include "bf_device_core.h"
#include "bf_endpoint_logic.h"
#include "bf_path_state.h"

BF_NS_BEGIN

// Mode specialisation: RX = 0 compiles the render modes only (path / range / time), RX = 1 the receive modes only,
// RX = 2 decides at run time (the one-kernel variant and the tail).  The receive branches carry the Wigner / phased-array
// / signal-model code; a shading kernel that cannot reach them allocates fewer registers.
template <int RX> BF_DEV bool mode_receive(const DLaunch &lp) { return (RX & kModeMask) == 2 ? lp.mode == BF_MODE_RECEIVE_RAW : (RX & kModeMask) == 1; }
// RX | kWide: the kernel variant for films / ADCs whose reconstruction filter is wider than a pixel (DLaunch::wide).  A variant
// of its own, not a branch: the filtered put's live values cost the box-filter kernels 3 % of wf_shade when both were compiled
// into one (profiles/r03_wide_filter_ab.txt), and every radar scene of the reference uses the box filter.

// ---------------------------------------------------------------------------
// path generation
// ---------------------------------------------------------------------------
template <int RX = 2> BF_DEV void generate_path(const DScene &sc0, const DLaunch &lp, uint64_t path_i, PathState &s) {
    const bool receive = mode_receive<RX>(lp);
    s.path_i = path_i;
    s.render = 0u;
    if (RX & kClass) s.cls = scene_miss_class(sc0);      // until the first intersection says otherwise (a slot's previous path leaves nothing behind)
    uint64_t seed = lp.seed, path_offset = lp.path_offset;
    if (lp.batch != 0u) {
        // batched launch: global index -> (render, local path); every render is an ordinary render of its own seed
        s.render = (uint32_t) (path_i / lp.batch_paths);
        path_i -= (uint64_t) s.render * lp.batch_paths;
        if (lp.roll) {                      // rolling sequence: the render's own seed and shard offset
            const DRoll &rr = lp.roll[s.render & (kRollRing - 1u)];
            seed = rr.seed;
            path_offset = rr.path_offset;
        } else if (lp.batch_seeds) {
            seed = lp.batch_seeds[s.render];
        }
    }
    const DScene sc = path_scene<RX>(sc0, lp, s.render);
    // per-path stream: sampler->seed(base_seed + path) (sampler.cpp:83-96)
    pcg_seed(s.rng, seed + path_offset + path_i);
    float fx = next_1d(s.rng), fy = next_1d(s.rng);
    float ax = .5f, ay = .5f;
    s.time = s.t_rx = s.lambda0 = s.phase = 0.f;
    s.dlambda = 0.f;
    bool film_ok = true, film_left = false, film_up = false;
    if (receive) {
        // receive_sample — integrator.cpp:1544-1572
        ax = next_1d(s.rng);
        ay = next_1d(s.rng);
        float time = c_sensor(sc).adc_sampling_start;
        if (c_sensor(sc).adc_sampling_time > 0.f)
            time += next_1d(s.rng) * c_sensor(sc).adc_sampling_time;
        else
            time = 0.f;
        float wl = next_1d(s.rng);
        s.t_rx = time;
        s.time = time;
        float w = receiver_sample_ray<RX>(sc, time, rare<RX>(lp.mix != 0u), wl, fx, fy, ax, ay, s.ro, s.rd, s.rmint, s.rmaxt, s.lambda0);
        s.aux = w;                 // receive has no path-length scalar: aux carries |ray_weight|'s operand
        if (rare<RX>(lp.resample != 0u)) s.dlambda = s.lambda0;      // the wavelength the receiver sampled (DLaunch::resample)
    } else {
        // render_sample — integrator.cpp:263-283
        if (rare<RX>(c_sensor(sc).type != BF_SENSOR_PERSPECTIVE && c_sensor(sc).type != BF_SENSOR_RADIANCEMETER)) {   // endpoint.h:241, perspective.cpp:130, radiancemeter.cpp:86-87
            ax = next_1d(s.rng);
            ay = next_1d(s.rng);
        }
        if (c_sensor(sc).shutter_open_time > 0.f) (void) next_1d(s.rng);
        (void) next_1d(s.rng);     // wavelength sample (consumed in RGB mode too)
        // position_sample = pos + next_2d; adjusted_position = position_sample / crop_size (integrator.cpp:263,276-278)
        uint32_t px = 0, py = 0;
        if (rare<RX>(lp.spp != 0u)) {
            const uint64_t q = (lp.path_offset + path_i) / lp.spp;
            px = (uint32_t) (q % lp.film_w);
            py = (uint32_t) (q / lp.film_w);
        }
        // film crop window (film.cpp:17-27): pixels are counted inside the crop, positions in the full film
        const uint32_t cx = rare<RX>(c_sensor(sc).crop_x != 0u) ? c_sensor(sc).crop_x : 0u, cy = rare<RX>(c_sensor(sc).crop_y != 0u) ? c_sensor(sc).crop_y : 0u;
        const float posx = (float) (px + cx) + fx, posy = (float) (py + cy) + fy;
        (void) sensor_sample_ray<RX>(sc, (posx - (float) cx) / (float) lp.film_w, (posy - (float) cy) / (float) lp.film_h, ax, ay, s.ro, s.rd,
                                     s.rmint, s.rmaxt);
        // ImageBlock::put, box branch (imageblock.cpp:113,166-172): pos = pos_ - (offset + .5) with the block's offset (the crop's,
        // plus whole blocks), the sample lands in pixel lo = ceil(pos - .5), i.e. the pixel it was drawn in or, when next_2d
        // returned exactly 0, its left / upper neighbour
        const float lx = __builtin_ceilf((posx - ((float) cx + .5f)) - .5f), ly = __builtin_ceilf((posy - ((float) cy + .5f)) - .5f);
        film_ok = lx >= 0.f && lx < (float) lp.film_w && ly >= 0.f && ly < (float) lp.film_h;
        film_left = lx < (float) px;
        film_up = ly < (float) py;
        s.aux = 0.f;
    }
    // the table's arrival form: the class of the path is its primary ray's direction's, whatever the ray goes on to hit (bf_arrival.h)
    if ((RX & kClass) && scene_class_arrival(sc0)) s.cls = scene_arrival_class(sc0, s.rd.x, s.rd.y, s.rd.z);
    s.throughput = 1.f;
    s.eta = 1.f;
    s.emission_weight = 1.f;
    s.result = 0.f;
    s.bs_pdf = 0.f;
    s.prev_p = mk(0, 0, 0);
    s.flags = (film_ok ? kFlagFilmOk : 0u) | (film_left ? kFlagFilmLeft : 0u) | (film_up ? kFlagFilmUp : 0u);
    s.n_rays = 1;
}

// ---------------------------------------------------------------------------
// one integrator iteration
// ---------------------------------------------------------------------------
struct ShadowReq {
    bool want;
    V3 o, d;
    float mint, maxt;
    float c;             // NEE contribution released by an unoccluded shadow ray
    float c_im;          // BF_MODE_RECEIVE_IQ: its imaginary part (c is the real part)
};

// BF_MODE_RECEIVE_IQ: unit phasor exp(-j 2 pi L / lambda) of an optical path of `length` metres at
// wavelength `lambda_nm`; the cycle count is reduced to its fractional part before the sine / cosine.
BF_DEV void path_phasor(float length, float lambda_nm, float &re, float &im) {
    float cycles = length / (lambda_nm * 1e-9f);
    float frac = cycles - __builtin_floorf(cycles);
    float s, c;
    bf_sincos(-6.28318530717958647692f * frac, s, c);
    re = c;
    im = s;
}
// Shape::doppler — src/librender/shape.cpp:375-389 (call sites commented out at the reference's HEAD:
// pathtimefrequency.cpp:141-144, 180-183): 2 dot(si.wi, m_velocity * Point3f(si.to_local(si.p))) / MTS_C * wavelength
BF_DEV float shape_doppler(const DScene &sc, const SI &si, float lambda_nm) {
    V3 q = xf_point(c_shapes(sc)[si.shape].velocity, to_local(si.sh, si.p));
    return 2.f * dot(si.wi, q) / sc.c * lambda_nm;
}

// Returns true if the path continues with a new closest-hit ray (s.ro/rd/...),
// false if it ended at the head of the iteration (film_put is due now).  When
// the BSDF sample kills the path (path.cpp:171-173) the function returns true
// with kFlagTermPending set and an empty ray interval: the film write has to
// wait for the shadow ray of this very iteration.
#if defined(BF_TAIL_PROF) || defined(BF_SHADE_PROF)
#define BF_VERTEX_PROF 1
#endif
#ifdef BF_VERTEX_PROF
struct ShadeProf {
    unsigned long long si, head, nee, bsdf;
};
#define BF_SHADEPROF_ARG , ShadeProf *spf = nullptr
#define BF_SHADEPROF_STAMP(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#else
#define BF_SHADEPROF_ARG
#define BF_SHADEPROF_STAMP(v)
#endif
// developer build (-DBF_SHADE_PROF, tools/shade_profile.py): how many lanes of a wave enter each section of wf_shade.
// SLP(sec, cond) sits in wave-uniform control flow right before `if (cond)`: one wave entry and popcount(cond) lanes.
#ifdef BF_SHADE_PROF
constexpr int kShadeProfSections = 32;
static __device__ unsigned long long g_lane_prof[2 * kShadeProfSections];      // [sec] = wave entries, [32 + sec] = lanes
#define BF_LANEPROF_ARG , bool lpf = false
#define SLP(sec, cond)                                                                      \
    do {                                                                                    \
        if (lpf) {                                                                          \
            const unsigned long long slp_b = __ballot(cond);                                \
            if (slp_b && (int) (threadIdx.x & 63) == __ffsll((long long) slp_b) - 1) {      \
                atomicAdd(&g_lane_prof[sec], 1ull);                                         \
                atomicAdd(&g_lane_prof[kShadeProfSections + (sec)], (unsigned long long) __popcll(slp_b)); \
            }                                                                               \
        }                                                                                   \
    } while (0)
#else
#define BF_LANEPROF_ARG
#define SLP(sec, cond)
#endif
// kAov: the first intersection's values into the side rows of the path's slot (bf_device.h: AovCtx), zeros for a miss.  Every path
// passes here exactly once, at its first vertex (a miss included), so this store is also what clears a regenerated slot's rows.
BF_DEV void aov_store(const AovCtx &av, bool valid, const SI &si, const SIGeom &g) {
    typedef __attribute__((address_space(1))) float *glb_f_ptr;
    glb_f_ptr q = (glb_f_ptr) av.rows + av.slot;
    const uint32_t n = av.stride;
    uint32_t r = 0u;
    const float z = 0.f;
#define BF_AOV_ROW(x) q[(size_t) (r++) * n] = valid ? (x) : z
    if (av.mask & 1u) { BF_AOV_ROW(si.t); }
    if (av.mask & 2u) { BF_AOV_ROW(si.p.x); BF_AOV_ROW(si.p.y); BF_AOV_ROW(si.p.z); }
    if (av.mask & 4u) { BF_AOV_ROW(g.u); BF_AOV_ROW(g.v); }
    if (av.mask & 8u) { BF_AOV_ROW(g.n.x); BF_AOV_ROW(g.n.y); BF_AOV_ROW(g.n.z); }
    if (av.mask & 16u) { BF_AOV_ROW(si.sh.n.x); BF_AOV_ROW(si.sh.n.y); BF_AOV_ROW(si.sh.n.z); }
    if (av.mask & 32u) { BF_AOV_ROW(g.dp_du.x); BF_AOV_ROW(g.dp_du.y); BF_AOV_ROW(g.dp_du.z); }
    if (av.mask & 64u) { BF_AOV_ROW(g.dp_dv.x); BF_AOV_ROW(g.dp_dv.y); BF_AOV_ROW(g.dp_dv.z); }
#undef BF_AOV_ROW
}
// ... and back, when the path's sample is put: the stored components by type (0 where the table names none of the type)
struct AovVals {
    float t, px, py, pz, u, v, nx, ny, nz, sx, sy, sz, ux, uy, uz, vx, vy, vz;
};
BF_DEV AovVals aov_load(const AovCtx &av) {
    typedef const __attribute__((address_space(1))) float *glb_cf_ptr;
    glb_cf_ptr q = (glb_cf_ptr) av.rows + av.slot;
    const uint32_t n = av.stride;
    uint32_t r = 0u;
    AovVals a = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#define BF_AOV_ROW(x) x = q[(size_t) (r++) * n]
    if (av.mask & 1u) { BF_AOV_ROW(a.t); }
    if (av.mask & 2u) { BF_AOV_ROW(a.px); BF_AOV_ROW(a.py); BF_AOV_ROW(a.pz); }
    if (av.mask & 4u) { BF_AOV_ROW(a.u); BF_AOV_ROW(a.v); }
    if (av.mask & 8u) { BF_AOV_ROW(a.nx); BF_AOV_ROW(a.ny); BF_AOV_ROW(a.nz); }
    if (av.mask & 16u) { BF_AOV_ROW(a.sx); BF_AOV_ROW(a.sy); BF_AOV_ROW(a.sz); }
    if (av.mask & 32u) { BF_AOV_ROW(a.ux); BF_AOV_ROW(a.uy); BF_AOV_ROW(a.uz); }
    if (av.mask & 64u) { BF_AOV_ROW(a.vx); BF_AOV_ROW(a.vy); BF_AOV_ROW(a.vz); }
#undef BF_AOV_ROW
    return a;
}
// the (up to three) floats of one table entry; duv_dx / duv_dy: zeros (interaction.h:635)
BF_DEV void aov_entry(const AovVals &a, uint32_t type, float &x, float &y, float &z) {
    x = y = z = 0.f;
    switch (type) {
        case BF_AOV_DEPTH: x = a.t; break;
        case BF_AOV_POSITION: x = a.px, y = a.py, z = a.pz; break;
        case BF_AOV_UV: x = a.u, y = a.v; break;
        case BF_AOV_GEO_NORMAL: x = a.nx, y = a.ny, z = a.nz; break;
        case BF_AOV_SH_NORMAL: x = a.sx, y = a.sy, z = a.sz; break;
        case BF_AOV_DP_DU: x = a.ux, y = a.uy, z = a.uz; break;
        case BF_AOV_DP_DV: x = a.vx, y = a.vy, z = a.vz; break;
        default: break;
    }
}
template <int RX = 2>
BF_DEV bool shade_vertex(const DScene &sc0, const DLaunch &lp, PathState &s, const Hit &hit, ShadowReq &sh,
                         uint32_t &c_bounces, const AovCtx &av BF_SHADEPROF_ARG BF_LANEPROF_ARG) {
    BF_SHADEPROF_STAMP(spf_t0);
    const DScene sc = path_scene<RX>(sc0, lp, s.render);
    const bool receive = mode_receive<RX>(lp);
    const bool is_range = !receive && lp.mode == BF_MODE_RANGE, is_time = rare<RX>(!receive && lp.mode == BF_MODE_TIME);
    const bool iq = receive && lp.iq != 0u;
    const bool phase_bins = rare<RX>(receive && lp.phase_bins != 0u);
    const bool doppler = rare<RX>(receive && lp.doppler != 0u);
    const uint32_t n_emit = (RX & kLean) ? 1u : sc.n_emitters;
    sh.want = false;
    SI si;
    const bool si_valid = hit.t != BF_INF;
    int emitter = -1;
    SLP(10, si_valid);
    bf_material mat;
    mat.type = ~0u;
    mat.back_material = 0u;
    SIGeom aov_g;      // kAov: the parts of the interaction only the AOVs read (the full surface interaction computes the same si)
    if (si_valid) {
        if (RX & kAov)
            make_si<true, RX>(sc, s.ro, s.rd, hit, si, &aov_g, path_shift(lp, s.render));
        else
            make_si<false, RX>(sc, s.ro, s.rd, hit, si, nullptr, path_shift(lp, s.render));
        emitter = si.emitter;
        mat = load_material(sc, si.material);      // issued here, waited for where NEE / BSDF sampling first read it
    }
#ifdef BF_VERTEX_PROF
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
    BF_SHADEPROF_STAMP(spf_t1);
    uint32_t depth = s.flags & kDepthMask;
    if (depth == 0) {
        // first intersection — path.cpp:115-117, pathlength.cpp:138-146,
        // pathtime.cpp:136-140, pathtimefrequency.cpp:131-153
        if (si_valid) s.flags |= kFlagValid;
        // the class of the path: its first intersection's shape, or the bin of that intersection's range rate along the primary ray, which
        // s.rd still is (bf_range_rate.h); the arrival form gave the path its class when it was generated
        if ((RX & kClass) && si_valid && !scene_class_arrival(sc)) {
            if (scene_class_range_rate(sc))
                s.cls = scene_range_rate_class(sc, si.shape, si.p.x, si.p.y, si.p.z, s.rd.x, s.rd.y, s.rd.z, hit.slot, hit.u, hit.v,
                                               (RX & kGeom) ? (uint64_t) s.render * lp.geom_stride : 0ull);
            else
                s.cls = scene_classes(sc)[si.shape];
        }
        if (RX & kAov) aov_store(av, si_valid, si, aov_g);      // ... or zeros: a miss never sees the values of the slot's previous path
        if (is_range) s.aux += si_valid ? si.t : 0.f;
        if (is_time) s.aux = si_valid ? si.t / lp.time_c : 0.f;
        if (si_valid && doppler) s.dlambda += shape_doppler(sc, si, s.lambda0);   // :141-144
        if (receive && si_valid) {                                 // ray.update_state(-si.t); si.time = ray.time
            s.time += -si.t / sc.c;
            if (phase_bins) s.phase = phase_update(s.phase, -si.t, sc.lambda_min, sc.lambda_max);
        }
        depth = 1;
    } else {
        // tail of the previous iteration — path.cpp:184-209, pathtimefrequency.cpp:363-399
        if (receive) {                                             // :368-371, also for a miss (Q3)
            s.time += -hit.t / sc.c;
            if (phase_bins) s.phase = phase_update(0.f, -hit.t, sc.lambda_min, sc.lambda_max);   // spawn_ray: phase restarts at 0
        }
        SLP(11, emitter >= 0);
        if (emitter >= 0) {
            CEmitter &e = c_emitters(sc)[(RX & kLean) ? 0 : emitter];      // lean: ONE emitter, a wave-uniform record
            float emitter_pdf = receive ? transmitter_pdf_direction<RX>(sc, e, s.prev_p, si.p, si.sh.n, s.lambda0)
                                        : emitter_pdf_direction<RX>(sc, e, s.prev_p, si.p, si.sh.n);
            if (n_emit != 1) emitter_pdf *= 1.f / (float) n_emit;
            s.emission_weight = mis_weight(s.bs_pdf, emitter_pdf);
        }
        if (is_range) s.aux += si_valid ? si.t : 0.f;
        if (is_time) s.aux += si_valid ? si.t / lp.time_c : 0.f;
        ++depth;
    }
    s.flags = (s.flags & ~kDepthMask) | (depth & kDepthMask);
    // head of iteration `depth` — path.cpp:121-145
    SLP(12, emitter >= 0);
    if (emitter >= 0) {
        CEmitter &e = c_emitters(sc)[(RX & kLean) ? 0 : emitter];
        if (doppler) s.dlambda += shape_doppler(sc, si, s.lambda0);               // :180-183
        float ev;
        if (receive)
            ev = transmitter_eval<RX>(sc, e, si, s.time, s.lambda0);
        else
            ev = ((RX & kLean) || e.type == BF_EMITTER_AREA) ? ((si.wi.z > 0.f) ? e.radiance : 0.f) : 0.f;
        float contrib = s.emission_weight * s.throughput * ev;
        if (iq) {
            // optical length receiver -> ... -> this transmitter point: c * (t_rx - retarded time)
            float re, im;
            path_phasor((s.t_rx - s.time) * sc.c, s.lambda0, re, im);
            s.result += contrib * re;
            s.phase += contrib * im;                               // imaginary accumulator (phase bins are off in IQ mode)
        } else {
            s.result += contrib;
        }
        if (is_range) s.aux += si_valid ? si.t : 0.f;              // pathlength.cpp:161
    }
    bool active = si_valid;
    if ((int) depth > lp.rr_depth) {
        float q = __builtin_fminf(s.throughput * sqr(s.eta), .95f);
        active = (next_1d(s.rng) < q) && active;
        s.throughput *= rcp(q);
    }
    if (depth >= (uint32_t) lp.max_depth || !active) return false;

    // TwoSidedBRDF with two nested BSDFs (twosided.cpp:108-178): the second one answers for incident directions below the surface
    if (rare<RX>(mat.back_material != 0u) && si.wi.z < 0.f) mat = load_material(sc, mat.back_material - 1u);
    ++c_bounces;
    BF_SHADEPROF_STAMP(spf_t2);
    SLP(13, true);                                        // lanes that survive to NEE + BSDF sampling
    SLP(15, mat.type == BF_BSDF_ROUGHCONDUCTOR);
    SLP(16, mat.type != BF_BSDF_ROUGHCONDUCTOR);
    if (bsdf_smooth(mat)) {
        // Scene::sample_emitter_direction / sample_transmitter_direction — scene.cpp:180-230, 249-299
        float sx = next_1d(s.rng), sy = next_1d(s.rng);
        DirSample ds;
        ds.d = mk(0, 0, 1);
        ds.pdf = 0.f;
        ds.dist = 0.f;
        ds.delta = false;
        float emitter_val = 0.f;
        if (n_emit >= 1) {
            uint32_t index = 0;
            float emitter_pdf = 1.f;
            if (n_emit > 1) {
                emitter_pdf = 1.f / (float) n_emit;
                index = min((uint32_t) (sx * (float) n_emit), n_emit - 1u);
                sx = (sx - index * emitter_pdf) * (float) n_emit;
            }
            CEmitter &e = c_emitters(sc)[index];
            if (receive)
                emitter_val = transmitter_sample_direction<RX>(sc, e, si.p, s.time, s.lambda0, sx, sy, ds);
            else
                emitter_val = emitter_sample_direction<RX>(sc, e, si.p, sx, sy, ds);
            if (n_emit > 1) {
                ds.pdf *= emitter_pdf;
                emitter_val *= rcp(emitter_pdf);
            }
        }
        SLP(14, ds.pdf != 0.f);
        if (ds.pdf != 0.f) {
            V3 wo = to_local(si.sh, ds.d);
            float bsdf_val, bsdf_pdf;
            bsdf_eval_pdf(mat, si.wi, wo, bsdf_val, bsdf_pdf);
            float mis = ds.delta ? 1.f : mis_weight(ds.pdf, bsdf_pdf);
            sh.c = mis * s.throughput * bsdf_val * emitter_val;
            sh.c_im = 0.f;
            if (iq) {
                float re, im;
                path_phasor((s.t_rx - s.time) * sc.c + ds.dist, s.lambda0, re, im);
                sh.c_im = sh.c * im;
                sh.c = sh.c * re;
            }
            sh.o = si.p;
            sh.d = ds.d;
            sh.mint = kRayEpsilon * (1.f + hmax_abs(si.p));
            sh.maxt = ds.dist * (1.f - kShadowEpsilon);
            sh.want = true;
            ++s.n_rays;
        }
        if (is_range) s.aux += si.t;                                // pathlength.cpp:209
    }
    BF_SHADEPROF_STAMP(spf_t3);
    (void) next_1d(s.rng);                                          // sample1 (unused by these BSDFs)
    float s2x = next_1d(s.rng), s2y = next_1d(s.rng);
    BSDFSample bs;
    float bsdf_val = bsdf_sample(mat, si.wi, s2x, s2y, bs);
    s.throughput = s.throughput * bsdf_val;
    if (s.throughput == 0.f) {
        s.flags |= kFlagTermPending;
        s.rmint = BF_INF;      // empty interval: no closest-hit query for this slot
        s.rmaxt = 0.f;
        return true;
    }
    s.eta *= bs.eta;
    // si.spawn_ray — interaction.h:61-64
    s.ro = si.p;
    s.rd = to_world(si.sh, bs.wo);
    s.rmint = (1.f + hmax_abs(si.p)) * kRayEpsilon;
    s.rmaxt = BF_INF;
    s.prev_p = si.p;
    s.bs_pdf = bs.pdf;
    ++s.n_rays;
#ifdef BF_VERTEX_PROF
    if (spf) {
        const unsigned long long spf_t4 = __builtin_amdgcn_s_memtime();
        spf->si += spf_t1 - spf_t0;
        spf->head += spf_t2 - spf_t1;
        spf->nee += spf_t3 - spf_t2;
        spf->bsdf += spf_t4 - spf_t3;
    }
#endif
    return true;
}

BF_NS_END  // namespace bfd
