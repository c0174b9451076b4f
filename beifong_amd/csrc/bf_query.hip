// Queries through the device functions the renders call, with their launchers (bf_launch.h; called by bf_api.cpp and
// bf_endpoints.cpp): batch ray intersection (bf_trace_kernel), the plugin-level BSDF, emitter and sensor queries, the microfacet and
// elementary-function probes, the developer's gather probe, and the engine's cosine on the host (bfk_host_cos).  Tests and tools
// only: none of it has a fast-arithmetic build (bf_ns.h), so this file is built once, exact.
// Built with -ffp-contract=off like every object here: bfk_host_cos is held bit for bit to the kernels' cosine.
#include <algorithm>

#include "bf_device_core.h"
#include "bf_launch.h"

#if BF_FAST
#error "bf_query.hip has no fast-arithmetic build"
#endif

BF_NS_BEGIN
// Scene::ray_intersect / ray_test over a batch of rays (tests, tools)
template <bool SPILL>
__global__ __launch_bounds__(kBlock) void bf_trace_kernel(DScene sc, uint64_t n, const float *__restrict__ rays,
                                                          int any_hit, float *__restrict__ out_t,
                                                          uint32_t *__restrict__ out_prim, uint32_t *__restrict__ out_shape,
                                                          float *__restrict__ out_uv, uint8_t *__restrict__ out_hit,
                                                          float *__restrict__ out_si) {
    __shared__ int s_stack[kStackDepth * kBlock];
    int *stack = s_stack + threadIdx.x;
    for (uint64_t i = (uint64_t) blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t) gridDim.x * kBlock) {
    const float *r = rays + 8 * i;
    V3 o = mk(r[0], r[1], r[2]), d = mk(r[4], r[5], r[6]);
    float mint = r[3], maxt = r[7];
    Hit h;
    uint32_t a = 0, b = 0;
    if (any_hit) {
        out_hit[i] = traverse<true, false, SPILL>(sc, o, d, mint, maxt, stack, h, a, b) ? 1 : 0;
    } else {
        bool valid = traverse<false, false, SPILL>(sc, o, d, mint, maxt, stack, h, a, b);
        if (out_t) out_t[i] = h.t;
        if (out_prim) out_prim[i] = valid ? h.prim : 0xffffffffu;
        if (out_shape) {
            uint32_t s = 0xffffffffu;
            if (valid) s = h.slot < 0 ? c_rects(sc)[-h.slot - 1].shape : __float_as_uint(sc.tris[kTriStride * (size_t) h.slot + 1].w);
            out_shape[i] = s;
        }
        if (out_uv) {
            out_uv[2 * i] = h.u;
            out_uv[2 * i + 1] = h.v;
        }
        if (out_si) {
            // SurfaceInteraction record of bf_ray_intersect (BF_SI_FLOATS); misses report t = +inf and zeros
            float *q = out_si + (size_t) BF_SI_FLOATS * i;
            for (int k = 0; k < BF_SI_FLOATS; ++k) q[k] = 0.f;
            q[0] = h.t;
            if (valid) {
                SI si;
                SIGeom g;
                make_si<true>(sc, o, d, h, si, &g);
                const V3 v[8] = {si.p, g.n, si.sh.n, si.sh.s, si.sh.t, si.wi, g.dp_du, g.dp_dv};
                for (int k = 0; k < 6; ++k) {
                    q[1 + 3 * k] = v[k].x;
                    q[2 + 3 * k] = v[k].y;
                    q[3 + 3 * k] = v[k].z;
                }
                q[19] = h.u;
                q[20] = h.v;
                for (int k = 6; k < 8; ++k) {
                    q[3 + 3 * k] = v[k].x;
                    q[4 + 3 * k] = v[k].y;
                    q[5 + 3 * k] = v[k].z;
                }
            }
        }
    }
    }
}
BF_NS_END  // namespace bfd

extern "C" hipError_t bfk_launch_trace(const bfd::DScene *sc, uint64_t n, const float *rays, int any_hit, float *out_t,
                                       uint32_t *out_prim, uint32_t *out_shape, float *out_uv, uint8_t *out_hit,
                                       float *out_si, hipStream_t stream) {
    unsigned grid = (unsigned) std::min<uint64_t>((n + bfd::kBlock - 1) / bfd::kBlock, sc->spill_stride / bfd::kBlock);
    if (grid == 0) return hipSuccess;
    if (sc->stack_need > (uint32_t) bfd::kStackDepth)
        hipLaunchKernelGGL(bfd::bf_trace_kernel<true>, dim3(grid), dim3(bfd::kBlock), 0, stream, *sc, n, rays, any_hit, out_t,
                           out_prim, out_shape, out_uv, out_hit, out_si);
    else
        hipLaunchKernelGGL(bfd::bf_trace_kernel<false>, dim3(grid), dim3(bfd::kBlock), 0, stream, *sc, n, rays, any_hit, out_t,
                           out_prim, out_shape, out_uv, out_hit, out_si);
    return hipGetLastError();
}

BF_NS_BEGIN
// Developer probe (tools/fetch_probe.py, profiles/README.md): what rocprofv3's FETCH_SIZE reports for the access patterns of
// this engine, on a table of known size that is read exactly once per launch.
//   MODE 0: streaming — thread g loads row g (16 B per lane, coalesced): every 128-byte line fully used by one wave
//   MODE 1: scattered rows — thread g loads row perm(g) (a bijection: an odd multiplier modulo the row count): every row
//           once, the eight rows of a line by eight different waves at different times (wf_trace's node / triangle fetches)
//   MODE 2: one 16-byte row per 128-byte line — thread g loads row 8 perm(g): 1/8 of the table's lines, each touched once
template <int MODE> __global__ void bf_gather_probe(const float4 *__restrict__ table, uint32_t n_rows, float4 *__restrict__ out) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t n = MODE == 2 ? n_rows / 8u : n_rows;
    if (g >= n) return;
    uint32_t row = g;
    if (MODE >= 1) row = (g * 2654435761u) & (n - 1u);      // n is a power of two, the multiplier odd: a permutation
    if (MODE == 2) row *= 8u;
    const float4 v = table[row];
    if (v.x == 12345.678f) out[g & 1023u] = v;      // (never true: keeps the load)
}
BF_NS_END  // namespace bfd
extern "C" hipError_t bfk_gather_probe(int mode, const float4 *table, uint32_t n_rows, float4 *out, hipStream_t stream) {
    const uint32_t n = mode == 2 ? n_rows / 8u : n_rows;
    const dim3 grid((n + 255u) / 256u), block(256);
    if (mode == 0) hipLaunchKernelGGL(bfd::bf_gather_probe<0>, grid, block, 0, stream, table, n_rows, out);
    else if (mode == 1) hipLaunchKernelGGL(bfd::bf_gather_probe<1>, grid, block, 0, stream, table, n_rows, out);
    else hipLaunchKernelGGL(bfd::bf_gather_probe<2>, grid, block, 0, stream, table, n_rows, out);
    return hipGetLastError();
}

/* Host-side evaluation of the engine's fp32 cosine (bf_device_math.h), used by scene setup so that
 * precomputed emitter constants follow the same specification as the kernels. */
extern "C" float bfk_host_cos(float x) { return bfd::bf_cos(x); }

BF_NS_BEGIN
__global__ void bf_elementary_kernel(int op, uint64_t n, const float *__restrict__ x, float *__restrict__ y) {
    uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float v = x[i], r;
    switch (op) {
        case 0: r = sin_cr(v); break;
        case 1: r = cos_cr(v); break;
        case 2: r = acos_cr(v); break;
        case 3: r = exp_cr(v); break;
        case 4: r = log_cr(v); break;
        case 5: r = erf_cr(v); break;
        default: r = tan_cr(v); break;
    }
    y[i] = r;
}
BF_NS_END  // namespace bfd

extern "C" hipError_t bfk_launch_elementary(int op, uint64_t n, const float *x, float *y) {
    unsigned grid = (unsigned) ((n + 255) / 256);
    hipLaunchKernelGGL(bfd::bf_elementary_kernel, dim3(grid), dim3(256), 0, 0, op, n, x, y);
    return hipGetLastError();
}

// Plugin-level queries (bf_bsdf_eval_pdf, bf_bsdf_sample, bf_emitter_sample_direction, bf_sensor_sample_ray): one lane per
// query through the device functions the renders call, general profile (V = 0), so every material, emitter and sensor type
// is reachable.  Inputs and outputs are the row layouts of include/beifong_hip.h.
BF_NS_BEGIN
enum { kQueryEvalPdf = 0, kQuerySample = 1, kQueryEmitter = 2, kQuerySensor = 3 };
template <int OP>
__global__ __launch_bounds__(256) void bf_query_kernel(DScene sc, uint64_t n, const uint32_t *__restrict__ materials,
                                                       uint32_t emitter, const float *__restrict__ in, float *__restrict__ out) {
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    if (OP == kQueryEvalPdf || OP == kQuerySample) {
        const float *q = in + 6 * i;
        const V3 wi = mk(q[0], q[1], q[2]);
        const uint32_t k = materials[i];
        float *o = out + (OP == kQueryEvalPdf ? 2 : 5) * i;
        if (k >= sc.n_materials) {      // the _device forms cannot refuse an index they only see here: NaN rows
            for (int c = 0; c < (OP == kQueryEvalPdf ? 2 : 5); ++c) o[c] = __builtin_nanf("");
            return;
        }
        bf_material mat = load_material(sc, k);
        // TwoSidedBRDF with two nested BSDFs (twosided.cpp:108-178), as the shading vertex selects it
        if (mat.back_material != 0u && wi.z < 0.f) mat = load_material(sc, mat.back_material - 1u);
        if (OP == kQueryEvalPdf) {
            float ev, pdf;
            bsdf_eval_pdf(mat, wi, mk(q[3], q[4], q[5]), ev, pdf);
            o[0] = ev;
            o[1] = pdf;
        } else {
            BSDFSample bs;
            const float w = bsdf_sample(mat, wi, q[4], q[5], bs);      // q[3]: sample1, unused by a single-lobe BSDF
            o[0] = bs.wo.x;
            o[1] = bs.wo.y;
            o[2] = bs.wo.z;
            o[3] = bs.pdf;
            o[4] = w;
        }
    } else if (OP == kQueryEmitter) {
        const float *q = in + 5 * i;
        const V3 ref_p = mk(q[0], q[1], q[2]);
        CEmitter &e = c_emitters(sc)[emitter];
        DirSample ds;
        const float spec = emitter_sample_direction<0>(sc, e, ref_p, q[3], q[4], ds);
        float pdf_dir = 0.f;
        if (e.type != BF_EMITTER_SPOT && e.type != BF_EMITTER_POINT) {
            CRect &rc = c_rects(sc)[e.rect];
            const V3 p = xf_point(rc.to_world, mk(q[3] * 2.f - 1.f, q[4] * 2.f - 1.f, 0.f));
            pdf_dir = emitter_pdf_direction<0>(sc, e, ref_p, p, mk(rc.n[0], rc.n[1], rc.n[2]));
        }
        float *o = out + 8 * i;
        o[0] = ds.d.x;
        o[1] = ds.d.y;
        o[2] = ds.d.z;
        o[3] = ds.dist;
        o[4] = ds.pdf;
        o[5] = ds.delta ? 1.f : 0.f;
        o[6] = spec;
        o[7] = pdf_dir;
    } else {
        const float *q = in + 4 * i;
        V3 ro, rd;
        float mint, maxt;
        float w = sensor_sample_ray<0>(sc, q[0], q[1], q[2], q[3], ro, rd, mint, maxt);
        // irradiancemeter.cpp:82: the path's sensor weight divides by the surface area (bf_film.h: film_put, the same expression)
        if (c_sensor(sc).type == BF_SENSOR_IRRADIANCEMETER) w = 1.f * kPi / c_rects(sc)[c_sensor(sc).rect].area;
        float *o = out + 9 * i;
        o[0] = ro.x;
        o[1] = ro.y;
        o[2] = ro.z;
        o[3] = mint;
        o[4] = rd.x;
        o[5] = rd.y;
        o[6] = rd.z;
        o[7] = w;
        o[8] = maxt;
    }
}

// MicrofacetDistribution unit access (bf_eval_microfacet; op numbering of the oracle's bfo_microfacet): in [n][8] = wi.xyz,
// m.xyz, s.xy; out [n][4]: op 0 eval(m), 1 pdf(wi, m), 2 smith_g1(v = m, m = wi), 3 sample(wi, s) -> m.xyz, pdf
__global__ __launch_bounds__(256) void bf_microfacet_kernel(int op, uint32_t type, float alpha_u, float alpha_v, uint32_t sample_visible,
                                                            uint64_t n, const float *__restrict__ in, float *__restrict__ out) {
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    bf_material mat = {};
    mat.distribution = type;
    mat.alpha_u = alpha_u;
    mat.alpha_v = alpha_v;
    mat.sample_visible = sample_visible;
    const Microfacet d = mf_make(mat);
    const float *q = in + 8 * i;
    const V3 wi = mk(q[0], q[1], q[2]), m = mk(q[3], q[4], q[5]);
    float r[4] = {0.f, 0.f, 0.f, 0.f};
    if (op == 0) {
        r[0] = mf_eval(d, m);
    } else if (op == 1) {
        r[0] = mf_pdf(d, wi, m);
    } else if (op == 2) {
        r[0] = mf_smith_g1(d, m, wi);
    } else {
        V3 ms;
        mf_sample(d, wi, q[6], q[7], ms, r[3]);
        r[0] = ms.x;
        r[1] = ms.y;
        r[2] = ms.z;
    }
    float *o = out + 4 * i;
    for (int c = 0; c < 4; ++c) o[c] = r[c];
}
BF_NS_END  // namespace bfd

static unsigned query_grid(uint64_t n) { return (unsigned) ((n + 255) / 256); }

extern "C" hipError_t bfk_launch_query(int op, const bfd::DScene *sc, uint64_t n, const uint32_t *materials, uint32_t emitter,
                                       const float *in, float *out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const dim3 grid(query_grid(n)), block(256);
    switch (op) {
        case bfd::kQueryEvalPdf:
            hipLaunchKernelGGL(bfd::bf_query_kernel<bfd::kQueryEvalPdf>, grid, block, 0, stream, *sc, n, materials, emitter, in, out);
            break;
        case bfd::kQuerySample:
            hipLaunchKernelGGL(bfd::bf_query_kernel<bfd::kQuerySample>, grid, block, 0, stream, *sc, n, materials, emitter, in, out);
            break;
        case bfd::kQueryEmitter:
            hipLaunchKernelGGL(bfd::bf_query_kernel<bfd::kQueryEmitter>, grid, block, 0, stream, *sc, n, materials, emitter, in, out);
            break;
        default:
            hipLaunchKernelGGL(bfd::bf_query_kernel<bfd::kQuerySensor>, grid, block, 0, stream, *sc, n, materials, emitter, in, out);
            break;
    }
    return hipGetLastError();
}

extern "C" hipError_t bfk_launch_microfacet(int op, uint32_t type, float alpha_u, float alpha_v, uint32_t sample_visible, uint64_t n,
                                            const float *in, float *out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bfd::bf_microfacet_kernel, dim3(query_grid(n)), dim3(256), 0, stream, op, type, alpha_u, alpha_v, sample_visible,
                       n, in, out);
    return hipGetLastError();
}
