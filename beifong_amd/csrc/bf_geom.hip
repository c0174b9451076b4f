// The kernels that move a scene's geometry, with their launchers (bf_launch.h; called by bf_mesh.cpp and bf_pose.cpp): mesh
// translation, the rigid transform, the refit of both trees level by level, node requantisation, the vertex gather of a deformation,
// skinning, morph targets and recomputed vertex normals (with their host twin, bfk_host_vertex_normals).  Geometry is shared by
// both arithmetic modes (bf_ns.h), so this file is built once, exact; it needs bf_device_core.h and nothing of the path logic.
// Built with -ffp-contract=off like every object here: the host functions below are held bit for bit to the kernels.
#include "bf_device_core.h"
#include "bf_launch.h"

#if BF_FAST
#error "bf_geom.hip has no fast-arithmetic build"
#endif

BF_NS_BEGIN
// The 64-byte copy of one four-wide node that wf_trace reads (bf_bvh.h: Node4Q): bf::quantise_node4 (bf_bvh.cpp) operation for
// operation, from the node's fp32 child boxes (rows 0..5) and child references (row 6).  Used after a mesh translation and after
// a rigid-motion refit.
BF_DEV void quantise_node4_dev(float4 lx, float4 ly, float4 lz, float4 hx, float4 hy, float4 hz, float4 refs, float4 *__restrict__ q) {
    const float cl[3][4] = {{lx.x, lx.y, lx.z, lx.w}, {ly.x, ly.y, ly.z, ly.w}, {lz.x, lz.y, lz.z, lz.w}};
    const float chh[3][4] = {{hx.x, hx.y, hx.z, hx.w}, {hy.x, hy.y, hy.z, hy.w}, {hz.x, hz.y, hz.z, hz.w}};
    const int child[4] = {__float_as_int(refs.x), __float_as_int(refs.y), __float_as_int(refs.z), __float_as_int(refs.w)};
    float nlo[3], scale[3];
    uint32_t exps = 0, qlo[3] = {0, 0, 0}, qhi[3] = {0, 0, 0};
    for (int a = 0; a < 3; ++a) {
        float lo = BF_INF, hi = -BF_INF;
        for (int k = 0; k < 4; ++k)
            if (child[k] != kNoNode) {
                lo = __builtin_fminf(lo, cl[a][k]);
                hi = __builtin_fmaxf(hi, chh[a][k]);
            }
        nlo[a] = lo;
        int e = 0;
        (void) __builtin_frexpf((hi - lo) * (1.f / 255.f), &e);
        e = max(-100, min(100, e));
        if (!(lo + 255.f * __builtin_ldexpf(1.f, e) >= hi)) ++e;
        scale[a] = __builtin_ldexpf(1.f, e);
        exps |= (uint32_t) (e + 127) << (8 * a);
        for (int k = 0; k < 4; ++k) {
            uint32_t ql = 255u, qh = 0u;
            if (child[k] != kNoNode) {
                const float inv = 1.f / scale[a];
                float fl = __builtin_floorf((cl[a][k] - lo) * inv), fh = __builtin_ceilf((chh[a][k] - lo) * inv);
                fl = __builtin_fminf(255.f, __builtin_fmaxf(0.f, fl));
                fh = __builtin_fminf(255.f, __builtin_fmaxf(0.f, fh));
                while (fl > 0.f && lo + fl * scale[a] > cl[a][k]) fl -= 1.f;
                while (fh < 255.f && lo + fh * scale[a] < chh[a][k]) fh += 1.f;
                ql = (uint32_t) fl;
                qh = (uint32_t) fh;
            }
            qlo[a] |= ql << (8 * k);
            qhi[a] |= qh << (8 * k);
        }
    }
    q[0] = make_float4(nlo[0], nlo[1], nlo[2], __uint_as_float(exps));
    q[1] = refs;
    q[2] = make_float4(__uint_as_float(qlo[0]), __uint_as_float(qlo[1]), __uint_as_float(qlo[2]), __uint_as_float(qhi[0]));
    q[3] = make_float4(__uint_as_float(qhi[1]), __uint_as_float(qhi[2]), 0.f, 0.f);
}

// bf_scene_translate_meshes: triangles and node boxes of the pristine copies shifted by `d`.
__global__ void bf_translate_kernel(const float4 *__restrict__ tris0, float4 *__restrict__ tris, uint32_t n_tri_rows,
                                    const float4 *__restrict__ nodes0, float4 *__restrict__ nodes, float4 *__restrict__ qnodes, uint32_t n_nodes,
                                    const float4 *__restrict__ wnodes0, float4 *__restrict__ wnodes, uint32_t n_wchildren,
                                    float dx, float dy, float dz) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_tri_rows) {                       // one float4 row (a vertex + tag) per thread
        float4 v = tris0[i];
        tris[i] = make_float4(v.x + dx, v.y + dy, v.z + dz, v.w);
    }
    if (i < n_nodes) {
        const float4 *s = nodes0 + 8u * i;
        float4 *o = nodes + 8u * i;
        float4 lx = s[0], ly = s[1], lz = s[2], hx = s[3], hy = s[4], hz = s[5];
        // shifted vertices are rounded to fp32 again (half an ulp each) and the fma slab test allows for
        // 2^-24 |origin| (bf_bvh.h): re-pad every box by 2.4e-7 of its largest shifted coordinate
        // an unused slot (kNoNode) keeps its inverted box (+inf, -inf) as it is: inf - 2.4e-7 inf would be NaN
        const float4 refs = s[6];
#define BF_SHIFT(L, H, D, K)                                                                                  \
    if (__float_as_int(refs.K) != kNoNode) {                                                                  \
        float lo = L.K + D, hi = H.K + D;                                                                     \
        float e = 2.4e-7f * __builtin_fmaxf(__builtin_fabsf(lo), __builtin_fabsf(hi));                        \
        L.K = lo - e;                                                                                         \
        H.K = hi + e;                                                                                         \
    }
        BF_SHIFT(lx, hx, dx, x) BF_SHIFT(lx, hx, dx, y) BF_SHIFT(lx, hx, dx, z) BF_SHIFT(lx, hx, dx, w)
        BF_SHIFT(ly, hy, dy, x) BF_SHIFT(ly, hy, dy, y) BF_SHIFT(ly, hy, dy, z) BF_SHIFT(ly, hy, dy, w)
        BF_SHIFT(lz, hz, dz, x) BF_SHIFT(lz, hz, dz, y) BF_SHIFT(lz, hz, dz, z) BF_SHIFT(lz, hz, dz, w)
#undef BF_SHIFT
        o[0] = lx; o[1] = ly; o[2] = lz; o[3] = hx; o[4] = hy; o[5] = hz;
        o[6] = refs;
        o[7] = s[7];
        if (qnodes) quantise_node4_dev(lx, ly, lz, hx, hy, hz, refs, qnodes + 4u * i);      // re-quantised for wf_trace
    }
    if (i < n_wchildren) {                      // one child record of a sixteen-wide node (bf_bvh.h: Node16), same re-padding
        const float4 a = wnodes0[2u * i], b = wnodes0[2u * i + 1u];
        const bool used = __float_as_int(b.z) != kNoNode;      // (an unused slot stays inverted, as above)
        float lo[3] = {a.x, a.y, a.z}, hi[3] = {a.w, b.x, b.y};
        const float d[3] = {dx, dy, dz};
        for (int k = 0; used && k < 3; ++k) {
            lo[k] += d[k];
            hi[k] += d[k];
            const float e = 2.4e-7f * __builtin_fmaxf(__builtin_fabsf(lo[k]), __builtin_fabsf(hi[k]));
            lo[k] -= e;
            hi[k] += e;
        }
        wnodes[2u * i] = make_float4(lo[0], lo[1], lo[2], hi[0]);
        wnodes[2u * i + 1u] = make_float4(hi[1], hi[2], b.z, b.w);
    }
}
BF_NS_END  // namespace bfd

extern "C" hipError_t bfk_launch_translate(const float4 *tris0, float4 *tris, uint32_t n_tri_rows, const float4 *nodes0,
                                           float4 *nodes, float4 *qnodes, uint32_t n_nodes, const float4 *wnodes0, float4 *wnodes,
                                           uint32_t n_wchildren, const float *d, hipStream_t stream) {
    uint32_t n = n_tri_rows > n_nodes ? n_tri_rows : n_nodes;
    n = n > n_wchildren ? n : n_wchildren;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(bfd::bf_translate_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, tris0, tris, n_tri_rows, nodes0, nodes,
                       qnodes, n_nodes, wnodes0, wnodes, n_wchildren, d[0], d[1], d[2]);
    return hipGetLastError();
}

BF_NS_BEGIN
// bf_scene_transform_meshes.  Step 1: every triangle slot from its pristine rows through its shape's rigid
// 3x4 [R | t] (xf: 16 floats per shape, the 12 of the matrix, then word 12 = 1 if the shape moves at all).
//   p' = fl(fl(fl(fl(r0 x) + fl(r1 y)) + fl(r2 z)) + t)   per row, every product and sum rounded (no FMA: __fmul_rn / __fadd_rn)
//   n' = R n                                              same order, without t, not renormalised
// The .w words (prim, shape, tag) stay; a shape whose entry is the identity keeps its rows bit for bit.
// Version dimension (bf_render_motion_batch_device: one geometry version per render): blockIdx.y = version v
// writes the rows `vstride` float4 rows further per version and reads its transforms `xf_stride` floats further; the single
// transform of bf_scene_transform_meshes is the launch with one version.
BF_DEV float3 rigid_apply(const float *__restrict__ m, float x, float y, float z, bool with_t) {
    float r[3];
    for (int k = 0; k < 3; ++k) {
        const float s = __fadd_rn(__fadd_rn(__fmul_rn(m[4 * k + 0], x), __fmul_rn(m[4 * k + 1], y)), __fmul_rn(m[4 * k + 2], z));
        r[k] = with_t ? __fadd_rn(s, m[4 * k + 3]) : s;
    }
    return make_float3(r[0], r[1], r[2]);
}

__global__ void bf_rigid_tris_kernel(const float4 *__restrict__ tris0, float4 *__restrict__ tris, const float4 *__restrict__ nrm0,
                                     float4 *__restrict__ nrm, uint32_t n_tris, const float *__restrict__ xf, uint64_t vstride, uint32_t xf_stride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tris) return;
    tris += vstride * blockIdx.y;
    if (nrm) nrm += vstride * blockIdx.y;
    xf += (size_t) xf_stride * blockIdx.y;
    const float4 *s = tris0 + kTriStride * i;
    float4 v[3] = {s[0], s[1], s[2]};
    const float *m = xf + 16u * __float_as_uint(v[1].w);
    const bool moves = m[12] != 0.f;
    if (moves)
        for (int j = 0; j < 3; ++j) {
            const float3 p = rigid_apply(m, v[j].x, v[j].y, v[j].z, true);
            v[j] = make_float4(p.x, p.y, p.z, v[j].w);
        }
    float4 *o = tris + kTriStride * i;
    o[0] = v[0];
    o[1] = v[1];
    o[2] = v[2];
    if (nrm) {
        for (int j = 0; j < 3; ++j) {
            float4 n = nrm0[3u * i + j];
            if (moves) {
                const float3 r = rigid_apply(m, n.x, n.y, n.z, false);
                n = make_float4(r.x, r.y, r.z, n.w);
            }
            nrm[3u * i + j] = n;
        }
    }
}

// the builder's padding (bf_bvh.cpp: Builder::pad) of an UNPADDED box; abs_pad = 2e-7 origin_scale
BF_DEV void refit_pad(float *lo, float *hi, float abs_pad) {
    float m = 0.f;
    for (int a = 0; a < 3; ++a)
        m = __builtin_fmaxf(m, __builtin_fmaxf(hi[a] - lo[a], __builtin_fmaxf(__builtin_fabsf(lo[a]), __builtin_fabsf(hi[a]))));
    const float e = 2e-6f * m + abs_pad + 1e-30f;
    for (int a = 0; a < 3; ++a) {
        lo[a] -= e;
        hi[a] += e;
    }
}
BF_DEV void refit_grow_tris(const float4 *__restrict__ tris, uint32_t first, uint32_t count, float *lo, float *hi) {
    for (uint32_t t = 0; t < count; ++t)
        for (int j = 0; j < 3; ++j) {
            const float4 p = tris[kTriStride * (first + t) + j];
            lo[0] = __builtin_fminf(lo[0], p.x), lo[1] = __builtin_fminf(lo[1], p.y), lo[2] = __builtin_fminf(lo[2], p.z);
            hi[0] = __builtin_fmaxf(hi[0], p.x), hi[1] = __builtin_fmaxf(hi[1], p.y), hi[2] = __builtin_fmaxf(hi[2], p.z);
        }
}
// union of the W unpadded child records of node `ref` (ubox: two float4 per child record, (lo.xyz, hi.x), (hi.yz, -, -))
template <int W> BF_DEV void refit_grow_node(const float4 *__restrict__ ubox, int32_t ref, float *lo, float *hi) {
    const float4 *c = ubox + 2u * W * (uint32_t) ref;
    for (int j = 0; j < W; ++j) {
        const float4 a = c[2 * j], b = c[2 * j + 1];
        lo[0] = __builtin_fminf(lo[0], a.x), lo[1] = __builtin_fminf(lo[1], a.y), lo[2] = __builtin_fminf(lo[2], a.z);
        hi[0] = __builtin_fmaxf(hi[0], a.w), hi[1] = __builtin_fmaxf(hi[1], b.x), hi[2] = __builtin_fmaxf(hi[2], b.y);
    }
}

// Step 2: one tree level of the four-wide nodes (bf_bvh.h: Node4), one thread per child slot.  A leaf child's box is the union
// of its <= kMaxLeaf moved triangles, an internal child's the union of that child's unpadded records, written by the launch of
// the level below.  The unpadded union goes to `ubox` (so padding never compounds up the tree), the padded one into the node.
// The references and empty slots (inverted boxes) come from the pristine node: the node written may be a fresh copy-on-write
// array, so every word of the slot's column is written.
__global__ void bf_refit4_kernel(const uint32_t *__restrict__ level, uint32_t n, const float4 *__restrict__ nodes0, float4 *__restrict__ nodes,
                                 float4 *__restrict__ ubox, const float4 *__restrict__ tris, float abs_pad, uint64_t vstride) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 4u * n) return;
    nodes += vstride * blockIdx.y;          // (version dimension: as bf_rigid_tris_kernel)
    ubox += vstride * blockIdx.y;
    tris += vstride * blockIdx.y;
    const uint32_t node = level[g >> 2], k = g & 3u;
    const float *src = reinterpret_cast<const float *>(nodes0 + 8u * node);
    float *row = reinterpret_cast<float *>(nodes + 8u * node);
    const int32_t ref = __float_as_int(src[24 + k]);
    float lo[3] = {BF_INF, BF_INF, BF_INF}, hi[3] = {-BF_INF, -BF_INF, -BF_INF};
    if (ref >= 0) {
        refit_grow_node<4>(ubox, ref, lo, hi);
    } else if (ref != kNoNode) {
        const uint32_t enc = ~(uint32_t) ref;
        refit_grow_tris(tris, enc >> 3, (enc & 7u) + 1u, lo, hi);
    }
    ubox[8u * node + 2u * k] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    ubox[8u * node + 2u * k + 1u] = make_float4(hi[1], hi[2], 0.f, 0.f);
    if (ref != kNoNode) {
        refit_pad(lo, hi, abs_pad);
    } else {
        for (int a = 0; a < 3; ++a) lo[a] = src[4 * a + k], hi[a] = src[4 * (3 + a) + k];
    }
    for (int a = 0; a < 3; ++a) {
        row[4 * a + k] = lo[a];
        row[4 * (3 + a) + k] = hi[a];
    }
    row[24 + k] = src[24 + k];
    row[28 + k] = src[28 + k];
}

// the same for the sixteen-wide nodes (bf_bvh.h: Node16): leaves hold up to kWideLeaf contiguous triangles
__global__ void bf_refit16_kernel(const uint32_t *__restrict__ level, uint32_t n, const float4 *__restrict__ wnodes0, float4 *__restrict__ wnodes,
                                  float4 *__restrict__ ubox, const float4 *__restrict__ tris, float abs_pad, uint64_t vstride) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 16u * n) return;
    wnodes += vstride * blockIdx.y;
    ubox += vstride * blockIdx.y;
    tris += vstride * blockIdx.y;
    const uint32_t node = level[g >> 4], k = g & 15u;
    const float4 a = wnodes0[32u * node + 2u * k], b = wnodes0[32u * node + 2u * k + 1u];
    float4 *c = wnodes + 32u * node + 2u * k;
    const int32_t ref = __float_as_int(b.z);
    float lo[3] = {BF_INF, BF_INF, BF_INF}, hi[3] = {-BF_INF, -BF_INF, -BF_INF};
    if (ref >= 0) {
        refit_grow_node<16>(ubox, ref, lo, hi);
    } else if (ref != kNoNode) {
        const uint32_t enc = ~(uint32_t) ref;
        refit_grow_tris(tris, enc >> 4, (enc & 15u) + 1u, lo, hi);
    }
    ubox[32u * node + 2u * k] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    ubox[32u * node + 2u * k + 1u] = make_float4(hi[1], hi[2], 0.f, 0.f);
    if (ref == kNoNode) {
        c[0] = a;
        c[1] = b;
        return;
    }
    refit_pad(lo, hi, abs_pad);
    c[0] = make_float4(lo[0], lo[1], lo[2], hi[0]);
    c[1] = make_float4(hi[1], hi[2], b.z, b.w);
}

// Step 3 (BF_QUANT_BVH=1 scenes): the quantised copies from the refitted fp32 nodes
__global__ void bf_requant_kernel(const float4 *__restrict__ nodes, float4 *__restrict__ qnodes, uint32_t n_nodes, uint64_t vstride) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_nodes) return;
    nodes += vstride * blockIdx.y;
    qnodes += vstride * blockIdx.y;
    const float4 *s = nodes + 8u * i;
    quantise_node4_dev(s[0], s[1], s[2], s[3], s[4], s[5], s[6], qnodes + 4u * i);
}
BF_NS_END  // namespace bfd

// The whole refit in stream order: the triangle transform, then one launch per level of each tree, deepest first
// (nodes0 / wnodes0: the pristine trees the topology is read from; lvl4 / lvl16: node indices grouped by depth, level d = [off[d], off[d + 1]) on the device, offsets on the host), then the
// re-quantisation.  The topology does not change, so the traversal stack bounds (stack_need, the spill columns) and the tail's
// row count that bf_scene_create derived from it stay valid.  n_versions > 1 (bf_render_motion_batch_device): every launch covers
// all versions at once (grid y = version; the outputs and scratch of version v lie v * vstride float4 rows after version 0's, its
// transforms v * xf_stride floats after the first table), so K versions cost the launches of one.
// steps 2 and 3 alone: both trees re-fitted over the triangle rows `tris` holds already, then the re-quantisation
static hipError_t launch_refit_levels(const float4 *tris, const float4 *nodes0, float4 *nodes, float4 *qnodes, uint32_t n_nodes,
                                      const uint32_t *lvl4, const uint32_t *lvl4_off, uint32_t n_lvl4, float4 *ubox4, const float4 *wnodes0,
                                      float4 *wnodes, const uint32_t *lvl16, const uint32_t *lvl16_off, uint32_t n_lvl16, float4 *ubox16,
                                      float abs_pad, uint32_t n_versions, uint64_t vstride, hipStream_t stream) {
    for (uint32_t d = n_lvl4; d-- > 0;) {
        const uint32_t n = lvl4_off[d + 1] - lvl4_off[d];
        if (n) hipLaunchKernelGGL(bfd::bf_refit4_kernel, dim3((4u * n + 255u) / 256u, n_versions), dim3(256), 0, stream, lvl4 + lvl4_off[d], n, nodes0,
                                  nodes, ubox4, (const float4 *) tris, abs_pad, vstride);
    }
    for (uint32_t d = n_lvl16; wnodes && d-- > 0;) {
        const uint32_t n = lvl16_off[d + 1] - lvl16_off[d];
        if (n) hipLaunchKernelGGL(bfd::bf_refit16_kernel, dim3((16u * n + 255u) / 256u, n_versions), dim3(256), 0, stream, lvl16 + lvl16_off[d], n,
                                  wnodes0, wnodes, ubox16, (const float4 *) tris, abs_pad, vstride);
    }
    if (qnodes && n_nodes)
        hipLaunchKernelGGL(bfd::bf_requant_kernel, dim3((n_nodes + 255u) / 256u, n_versions), dim3(256), 0, stream, (const float4 *) nodes, qnodes,
                           n_nodes, vstride);
    return hipGetLastError();
}

extern "C" hipError_t bfk_launch_rigid(const float4 *tris0, float4 *tris, const float4 *nrm0, float4 *nrm, uint32_t n_tris,
                                       const float *xf, const float4 *nodes0, float4 *nodes, float4 *qnodes, uint32_t n_nodes, const uint32_t *lvl4,
                                       const uint32_t *lvl4_off, uint32_t n_lvl4, float4 *ubox4, const float4 *wnodes0, float4 *wnodes, const uint32_t *lvl16,
                                       const uint32_t *lvl16_off, uint32_t n_lvl16, float4 *ubox16, float abs_pad, uint32_t n_versions,
                                       uint64_t vstride, uint32_t xf_stride, hipStream_t stream) {
    if (n_tris == 0 || n_versions == 0) return hipSuccess;
    if (n_versions > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bfd::bf_rigid_tris_kernel, dim3((n_tris + 255u) / 256u, n_versions), dim3(256), 0, stream, tris0, tris, nrm0, nrm, n_tris,
                       xf, vstride, xf_stride);
    return launch_refit_levels(tris, nodes0, nodes, qnodes, n_nodes, lvl4, lvl4_off, n_lvl4, ubox4, wnodes0, wnodes, lvl16, lvl16_off, n_lvl16,
                               ubox16, abs_pad, n_versions, vstride, stream);
}

BF_NS_BEGIN
// bf_scene_update_vertices / bf_render_deform_batch_device.  One thread per triangle slot (leaf order), grid y =
// version, `vstride` as bf_rigid_tris_kernel.  corners[slot] = the slot's three vertex indices within its shape and the shape's
// index; src[shape] says where the caller's arrays of that shape lie (pos == nullptr: the shape does not deform).
//   deforming slot : the row is the three positions (and, where given, the three normals) of version v, float for float
//   any other slot : the base row
// then, where `xf` is given (a batch: per version and shape, as bf_rigid_tris_kernel), the shape's rigid [R | t] by rigid_apply —
// the arithmetic of a transform call on the gathered rows.  The .w words are the base's.  `tris` may be `tris0` itself (the
// single update writes the base in place, one version): every lane reads its own rows before it writes them.
// Every gathered position must be finite with |c| <= bound and every gathered normal finite; a slot that fails keeps its base
// row, and its wave adds the number of such slots to bad[0] with ONE atomic (bad[1] = some failing shape + 1).
__global__ __launch_bounds__(256) void bf_deform_tris_kernel(const uint4 *__restrict__ corners, const DDeformSrc *__restrict__ src,
                                                             const float4 *tris0, float4 *tris, const float4 *nrm0, float4 *nrm,
                                                             uint32_t n_tris, const float *__restrict__ xf, uint64_t vstride,
                                                             uint32_t xf_stride, float bound, uint32_t *__restrict__ bad) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, ver = blockIdx.y;
    bool viol = false;
    uint32_t shape = 0;
    if (i < n_tris) {
        const uint4 c = corners[i];                       // one 16-byte load
        shape = c.w;
        const DDeformSrc s = src[shape];
        const float4 *b = tris0 + kTriStride * i;
        float4 *o = tris + vstride * ver + kTriStride * i;
        float4 v[3] = {b[0], b[1], b[2]};
        float4 n[3];
        const float4 *nb = nrm0 + 3u * i;
        float4 *no = nrm ? nrm + vstride * ver + 3u * i : nullptr;
        if (nrm)
            for (int j = 0; j < 3; ++j) n[j] = nb[j];
        bool changed = false;
        if (s.pos) {
            // the nine (eighteen) scattered loads are issued before the first use
            const float *p = s.pos + (size_t) ver * 3u * s.nv;
            const float *p0 = p + 3u * c.x, *p1 = p + 3u * c.y, *p2 = p + 3u * c.z;
            const float g[9] = {p0[0], p0[1], p0[2], p1[0], p1[1], p1[2], p2[0], p2[1], p2[2]};
            float h[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const bool with_n = nrm && s.nrm;
            if (with_n) {
                const float *q = s.nrm + (size_t) ver * 3u * s.nv;
                const float *q0 = q + 3u * c.x, *q1 = q + 3u * c.y, *q2 = q + 3u * c.z;
                h[0] = q0[0], h[1] = q0[1], h[2] = q0[2], h[3] = q1[0], h[4] = q1[1], h[5] = q1[2], h[6] = q2[0], h[7] = q2[1], h[8] = q2[2];
            }
            bool ok = true;
            for (int k = 0; k < 9; ++k) ok = ok && (__builtin_fabsf(g[k]) <= bound) && (__builtin_fabsf(h[k]) < BF_INF);      // false for NaN
            if (ok) {
                for (int j = 0; j < 3; ++j) {
                    v[j] = make_float4(g[3 * j], g[3 * j + 1], g[3 * j + 2], v[j].w);
                    if (with_n) n[j] = make_float4(h[3 * j], h[3 * j + 1], h[3 * j + 2], n[j].w);
                }
                changed = true;
            } else {
                viol = true;
            }
        }
        if (xf) {
            const float *m = xf + (size_t) xf_stride * ver + 16u * shape;
            if (m[12] != 0.f) {
                for (int j = 0; j < 3; ++j) {
                    const float3 p = rigid_apply(m, v[j].x, v[j].y, v[j].z, true);
                    v[j] = make_float4(p.x, p.y, p.z, v[j].w);
                    if (nrm) {
                        const float3 r = rigid_apply(m, n[j].x, n[j].y, n[j].z, false);
                        n[j] = make_float4(r.x, r.y, r.z, n[j].w);
                    }
                }
                changed = true;
            }
        }
        if (changed || o != b) {
            o[0] = v[0];
            o[1] = v[1];
            o[2] = v[2];
        }
        if (nrm && (changed || no != nb))
            for (int j = 0; j < 3; ++j) no[j] = n[j];
    }
    const unsigned long long vm = __ballot(viol);
    if (vm != 0ull && viol && (__ffsll(vm) - 1) == (int) (threadIdx.x & 63u)) {
        atomicAdd(bad, (uint32_t) __popcll(vm));
        bad[1] = shape + 1u;
    }
}
BF_NS_END  // namespace bfd

// The vertex gather alone (bf_scene_update_vertices: the output is the handle's base, bfk_launch_rigid follows with its pose) ...
extern "C" hipError_t bfk_launch_deform_tris(const uint4 *corners, const bfd::DDeformSrc *src, const float4 *tris0, float4 *tris, const float4 *nrm0,
                                             float4 *nrm, uint32_t n_tris, const float *xf, uint32_t n_versions, uint64_t vstride,
                                             uint32_t xf_stride, float bound, uint32_t *bad, hipStream_t stream) {
    if (n_tris == 0 || n_versions == 0) return hipSuccess;
    if (n_versions > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bfd::bf_deform_tris_kernel, dim3((n_tris + 255u) / 256u, n_versions), dim3(256), 0, stream, corners, src, tris0, tris, nrm0,
                       nrm, n_tris, xf, vstride, xf_stride, bound, bad);
    return hipGetLastError();
}
BF_NS_BEGIN
// The velocity rows of bf_scene_set_velocity_mode (bf_velocity.h): three float4 per triangle slot, the world-space
// velocity of each corner in face order (.w = 0).  One thread per triangle slot, grid y = version, `vstride` as bf_deform_tris_kernel.
// modes[shape] = (the bits of the shape's BF_VELOCITY_* mode, its dt).  Version v differences the triangle rows `prev` + vstride pv and
// `next` + vstride nv, (pv, nv) = (v, v + 1), or (tail_prev, tail_next) for the last version of the launch:
//   BF_VELOCITY_DIFFERENCE : fl(fl(next - prev) / dt) per component (bfvel::corner)
//   BF_VELOCITY_VERTEX     : the slot's rows of `own`, the handle's explicit field (the same for every version)
//   BF_VELOCITY_TWIST      : zeros (never read), or nothing where `own` is the output itself (the handle's rows: one version)
__global__ __launch_bounds__(256) void bf_velocity_diff_kernel(const float4 *__restrict__ prev, const float4 *__restrict__ next, float4 *vel,
                                                               const float4 *own, uint32_t n_tris, const float2 *__restrict__ modes,
                                                               uint64_t vstride, uint32_t tail_prev, uint32_t tail_next) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, ver = blockIdx.y;
    if (i >= n_tris) return;
    const bool last = ver + 1u == gridDim.y;
    const float4 *a = prev + vstride * (last ? tail_prev : ver) + kTriStride * (size_t) i;
    const float4 *b = next + vstride * (last ? tail_next : ver + 1u) + kTriStride * (size_t) i;
    float4 *o = vel + vstride * ver + bfvel::kRowsPerSlot * (size_t) i;
    const float4 *w = own ? own + bfvel::kRowsPerSlot * (size_t) i : nullptr;
    const float4 b0 = b[0], b1 = b[1], b2 = b[2];
    const float2 md = modes[__float_as_uint(b1.w)];
    const uint32_t mode = __float_as_uint(md.x);
    if (mode == bfvel::kDifference) {
        const float4 a0 = a[0], a1 = a[1], a2 = a[2];
        const float dt = md.y;
        o[0] = make_float4(bfvel::corner(a0.x, b0.x, dt), bfvel::corner(a0.y, b0.y, dt), bfvel::corner(a0.z, b0.z, dt), 0.f);
        o[1] = make_float4(bfvel::corner(a1.x, b1.x, dt), bfvel::corner(a1.y, b1.y, dt), bfvel::corner(a1.z, b1.z, dt), 0.f);
        o[2] = make_float4(bfvel::corner(a2.x, b2.x, dt), bfvel::corner(a2.y, b2.y, dt), bfvel::corner(a2.z, b2.z, dt), 0.f);
    } else if (w != o) {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        const bool copy = mode == bfvel::kVertex && w;
        const float4 r0 = copy ? w[0] : z, r1 = copy ? w[1] : z, r2 = copy ? w[2] : z;
        o[0] = r0;
        o[1] = r1;
        o[2] = r2;
    }
}
// bf_scene_set_vertex_velocities: the rows of every slot of shape `shape` from the per-vertex field `field` ([n_vertices][3]; nullptr:
// zeros) through the corner table, as bf_deform_tris_kernel gathers positions; every other slot's rows stay.
__global__ __launch_bounds__(256) void bf_velocity_gather_kernel(const uint4 *__restrict__ corners, const float4 *__restrict__ tris,
                                                                 const float *__restrict__ field, uint32_t shape, float4 *vel, uint32_t n_tris) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tris || __float_as_uint(tris[kTriStride * (size_t) i + 1].w) != shape) return;
    float4 *o = vel + bfvel::kRowsPerSlot * (size_t) i;
    float g[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (field) {
        const uint4 c = corners[i];
        const float *p0 = field + 3u * (size_t) c.x, *p1 = field + 3u * (size_t) c.y, *p2 = field + 3u * (size_t) c.z;
        g[0] = p0[0], g[1] = p0[1], g[2] = p0[2], g[3] = p1[0], g[4] = p1[1], g[5] = p1[2], g[6] = p2[0], g[7] = p2[1], g[8] = p2[2];
    }
    for (int j = 0; j < 3; ++j) o[j] = make_float4(g[3 * j], g[3 * j + 1], g[3 * j + 2], 0.f);
}
BF_NS_END  // namespace bfd

extern "C" hipError_t bfk_launch_velocity_diff(const float4 *prev, const float4 *next, float4 *vel, const float4 *own, uint32_t n_tris,
                                               const float2 *modes, uint32_t n_versions, uint64_t vstride, uint32_t tail_prev, uint32_t tail_next,
                                               hipStream_t stream) {
    if (n_tris == 0 || n_versions == 0) return hipSuccess;
    if (n_versions > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bfd::bf_velocity_diff_kernel, dim3((n_tris + 255u) / 256u, n_versions), dim3(256), 0, stream, prev, next, vel, own, n_tris,
                       modes, vstride, tail_prev, tail_next);
    return hipGetLastError();
}
extern "C" hipError_t bfk_launch_velocity_gather(const uint4 *corners, const float4 *tris, const float *field, uint32_t shape, float4 *vel,
                                                 uint32_t n_tris, hipStream_t stream) {
    if (n_tris == 0) return hipSuccess;
    hipLaunchKernelGGL(bfd::bf_velocity_gather_kernel, dim3((n_tris + 255u) / 256u), dim3(256), 0, stream, corners, tris, field, shape, vel, n_tris);
    return hipGetLastError();
}

// ... and the refit of both trees behind it (bf_render_deform_batch_device: gather + rigid transform in one pass over the rows, then
// the level kernels with the version dimension, as bfk_launch_rigid runs them)
extern "C" hipError_t bfk_launch_refit(const float4 *tris, const float4 *nodes0, float4 *nodes, float4 *qnodes, uint32_t n_nodes, const uint32_t *lvl4,
                                       const uint32_t *lvl4_off, uint32_t n_lvl4, float4 *ubox4, const float4 *wnodes0, float4 *wnodes,
                                       const uint32_t *lvl16, const uint32_t *lvl16_off, uint32_t n_lvl16, float4 *ubox16, float abs_pad,
                                       uint32_t n_versions, uint64_t vstride, hipStream_t stream) {
    if (n_versions == 0) return hipSuccess;
    if (n_versions > 65535u) return hipErrorInvalidValue;
    return launch_refit_levels(tris, nodes0, nodes, qnodes, n_nodes, lvl4, lvl4_off, n_lvl4, ubox4, wnodes0, wnodes, lvl16, lvl16_off, n_lvl16,
                               ubox16, abs_pad, n_versions, vstride, stream);
}

BF_NS_BEGIN
// bf_scene_pose_skin / bf_render_skin_batch_device: linear-blend skinning of one mesh shape.  One thread per vertex,
// grid y = version: version v reads its bone table (n_bones 3x4 matrices, at most 256: 12 KiB) `bone_stride` floats further and
// writes its vertices `vstride` floats further.  With q_k = rigid_apply(bone[index_k], rest) for the vertex's four slots,
//   p' = fl(fl(fl(fl(w0 q_0) + fl(w1 q_1)) + fl(w2 q_2)) + fl(w3 q_3))   per coordinate, every product and sum rounded (no FMA)
//   n' = the same without the bones' translations, on the rest normal, not renormalised
// All four terms are always evaluated: a zero weight still multiplies its bone's result.  The output is a plain [nv][3] array per
// version, which bf_deform_tris_kernel gathers (and checks against the bound the host derived) like a caller's own.
BF_DEV float3 skin_blend(const float *sb, uint4 ix, float4 w, float x, float y, float z, bool with_t) {
    const float3 q0 = rigid_apply(sb + 12u * ix.x, x, y, z, with_t), q1 = rigid_apply(sb + 12u * ix.y, x, y, z, with_t);
    const float3 q2 = rigid_apply(sb + 12u * ix.z, x, y, z, with_t), q3 = rigid_apply(sb + 12u * ix.w, x, y, z, with_t);
    const float a[3][4] = {{q0.x, q1.x, q2.x, q3.x}, {q0.y, q1.y, q2.y, q3.y}, {q0.z, q1.z, q2.z, q3.z}};
    float r[3];
    for (int c = 0; c < 3; ++c)
        r[c] = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(w.x, a[c][0]), __fmul_rn(w.y, a[c][1])), __fmul_rn(w.z, a[c][2])), __fmul_rn(w.w, a[c][3]));
    return make_float3(r[0], r[1], r[2]);
}

__global__ __launch_bounds__(256) void bf_skin_vertices_kernel(const float *__restrict__ rest_pos, const float *__restrict__ rest_nrm,
                                                               const uint4 *__restrict__ index, const float4 *__restrict__ weight, uint32_t nv,
                                                               const float *__restrict__ bones, uint32_t n_bones, uint32_t bone_stride,
                                                               float *__restrict__ pos, float *__restrict__ nrm, uint64_t vstride) {
    __shared__ float sb[256 * 12];
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, ver = blockIdx.y;
    const bool live = v < nv;
    // the lane's own loads are issued before the table's, all of them before the barrier
    uint4 ix = make_uint4(0u, 0u, 0u, 0u);
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    float x[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
    if (live) {
        ix = index[v];        // one 16-byte load each
        w = weight[v];
        for (int c = 0; c < 3; ++c) x[c] = rest_pos[3u * (size_t) v + c];
        if (rest_nrm)
            for (int c = 0; c < 3; ++c) n[c] = rest_nrm[3u * (size_t) v + c];
    }
    const float *b = bones + (size_t) bone_stride * ver;
    for (uint32_t i = threadIdx.x; i < n_bones * 12u; i += 256u) sb[i] = b[i];
    __syncthreads();
    if (!live) return;
    const size_t o = (size_t) vstride * ver + 3u * (size_t) v;
    const float3 p = skin_blend(sb, ix, w, x[0], x[1], x[2], true);
    pos[o] = p.x, pos[o + 1] = p.y, pos[o + 2] = p.z;
    if (rest_nrm) {
        const float3 r = skin_blend(sb, ix, w, n[0], n[1], n[2], false);
        nrm[o] = r.x, nrm[o + 1] = r.y, nrm[o + 2] = r.z;
    }
}
BF_NS_END  // namespace bfd

// n_versions poses of one skinned shape: bones [n_versions][n_bones][12] (device) -> pos (and nrm, if the skin has rest normals),
// [n_versions][nv][3] each
extern "C" hipError_t bfk_launch_skin_vertices(const float *rest_pos, const float *rest_nrm, const uint4 *index, const float4 *weight, uint32_t nv,
                                               const float *bones, uint32_t n_bones, float *pos, float *nrm, uint32_t n_versions,
                                               hipStream_t stream) {
    if (nv == 0 || n_versions == 0) return hipSuccess;
    if (n_versions > 65535u || n_bones == 0 || n_bones > 256u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bfd::bf_skin_vertices_kernel, dim3((nv + 255u) / 256u, n_versions), dim3(256), 0, stream, rest_pos, rest_nrm, index, weight,
                       nv, bones, n_bones, n_bones * 12u, pos, nrm, (uint64_t) 3u * nv);
    return hipGetLastError();
}

BF_NS_BEGIN
// Dual-quaternion skinning (BF_SKIN_DUAL_QUATERNION): bf_skin_vertices_kernel's layout with another blend.  The bone
// table holds one unit dual quaternion per bone, 8 floats (real w x y z, dual w x y z: bf_pose.cpp converts the caller's 3x4 on the
// host), at most 256: 8 KiB of LDS, read as two 16-byte rows per slot.  fp32, every operation rounded (no FMA, IEEE division and
// square root; the square root is the builtin for vn_sqrt's reason, below).  Per vertex, with slots k = 0..3:
//   p   = the slot of largest weight, the first among equals;   s_k = -1 if dot(D_k.real, D_p.real) < 0, else +1
//   b   = ((s0 w0 D_0 + s1 w1 D_1) + s2 w2 D_2) + s3 w3 D_3     per component over all eight, all four terms always evaluated
//   r   = b.real / |b.real|,  e = b.dual / |b.real|             (dot and |.|^2 are ((a0 b0 + a1 b1) + a2 b2) + a3 b3)
//   rotate(r, v) = (v + rw t) + cross(r.xyz, t)  with  t = 2 cross(r.xyz, v),   cross(a, b).x = fl(fl(ay bz) - fl(az by))
//   x'  = rotate(r, x) + 2 ((rw e.xyz - ew r.xyz) + cross(r.xyz, e.xyz))
//   n'  = rotate(r, n)                                          no translation, not renormalised
// s_k w_k is exact (a sign), and so are the products by 2.
struct DqBlend {
    float r[4], e[4];
};
BF_DEV float dq_dot4(float4 a, float4 b) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(a.x, b.x), __fmul_rn(a.y, b.y)), __fmul_rn(a.z, b.z)), __fmul_rn(a.w, b.w));
}
BF_DEV float dq_sum4(const float c[4], float d0, float d1, float d2, float d3) {
    return __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c[0], d0), __fmul_rn(c[1], d1)), __fmul_rn(c[2], d2)), __fmul_rn(c[3], d3));
}
BF_DEV DqBlend dq_blend(const float4 *sq, uint4 ix, float4 w) {
    const float4 R0 = sq[2u * ix.x], R1 = sq[2u * ix.y], R2 = sq[2u * ix.z], R3 = sq[2u * ix.w];
    const float4 E0 = sq[2u * ix.x + 1u], E1 = sq[2u * ix.y + 1u], E2 = sq[2u * ix.z + 1u], E3 = sq[2u * ix.w + 1u];
    float4 P = R0;
    float wp = w.x;
    if (w.y > wp) P = R1, wp = w.y;
    if (w.z > wp) P = R2, wp = w.z;
    if (w.w > wp) P = R3, wp = w.w;
    const float c[4] = {dq_dot4(R0, P) < 0.f ? -w.x : w.x, dq_dot4(R1, P) < 0.f ? -w.y : w.y, dq_dot4(R2, P) < 0.f ? -w.z : w.z,
                        dq_dot4(R3, P) < 0.f ? -w.w : w.w};
    const float4 br = make_float4(dq_sum4(c, R0.x, R1.x, R2.x, R3.x), dq_sum4(c, R0.y, R1.y, R2.y, R3.y), dq_sum4(c, R0.z, R1.z, R2.z, R3.z),
                                  dq_sum4(c, R0.w, R1.w, R2.w, R3.w));
    const float bd[4] = {dq_sum4(c, E0.x, E1.x, E2.x, E3.x), dq_sum4(c, E0.y, E1.y, E2.y, E3.y), dq_sum4(c, E0.z, E1.z, E2.z, E3.z),
                         dq_sum4(c, E0.w, E1.w, E2.w, E3.w)};
    const float len = __builtin_sqrtf(dq_dot4(br, br));
    DqBlend q;
    q.r[0] = __fdiv_rn(br.x, len), q.r[1] = __fdiv_rn(br.y, len), q.r[2] = __fdiv_rn(br.z, len), q.r[3] = __fdiv_rn(br.w, len);
    for (int j = 0; j < 4; ++j) q.e[j] = __fdiv_rn(bd[j], len);
    return q;
}
// cross(a, b), each component fl(fl(ay bz) - fl(az by))
BF_DEV float3 dq_cross(float ax, float ay, float az, float bx, float by, float bz) {
    return make_float3(__fsub_rn(__fmul_rn(ay, bz), __fmul_rn(az, by)), __fsub_rn(__fmul_rn(az, bx), __fmul_rn(ax, bz)),
                       __fsub_rn(__fmul_rn(ax, by), __fmul_rn(ay, bx)));
}
BF_DEV float3 dq_rotate(const DqBlend &q, float x, float y, float z) {
    const float3 h = dq_cross(q.r[1], q.r[2], q.r[3], x, y, z);
    const float3 t = make_float3(__fmul_rn(2.f, h.x), __fmul_rn(2.f, h.y), __fmul_rn(2.f, h.z));
    const float3 u = dq_cross(q.r[1], q.r[2], q.r[3], t.x, t.y, t.z);
    return make_float3(__fadd_rn(__fadd_rn(x, __fmul_rn(q.r[0], t.x)), u.x), __fadd_rn(__fadd_rn(y, __fmul_rn(q.r[0], t.y)), u.y),
                       __fadd_rn(__fadd_rn(z, __fmul_rn(q.r[0], t.z)), u.z));
}
BF_DEV float3 dq_point(const DqBlend &q, float x, float y, float z) {
    const float3 p = dq_rotate(q, x, y, z), u = dq_cross(q.r[1], q.r[2], q.r[3], q.e[1], q.e[2], q.e[3]);
    const float tx = __fmul_rn(2.f, __fadd_rn(__fsub_rn(__fmul_rn(q.r[0], q.e[1]), __fmul_rn(q.e[0], q.r[1])), u.x));
    const float ty = __fmul_rn(2.f, __fadd_rn(__fsub_rn(__fmul_rn(q.r[0], q.e[2]), __fmul_rn(q.e[0], q.r[2])), u.y));
    const float tz = __fmul_rn(2.f, __fadd_rn(__fsub_rn(__fmul_rn(q.r[0], q.e[3]), __fmul_rn(q.e[0], q.r[3])), u.z));
    return make_float3(__fadd_rn(p.x, tx), __fadd_rn(p.y, ty), __fadd_rn(p.z, tz));
}
// the bone table of version `ver` into LDS: n_bones rows of two float4 (the staged table is 16-byte aligned: bf_pose.cpp)
BF_DEV void dq_table_load(float4 *sq, const float *bones, uint32_t n_bones, uint32_t bone_stride, uint32_t ver) {
    const float4 *b = reinterpret_cast<const float4 *>(bones + (size_t) bone_stride * ver);
    for (uint32_t i = threadIdx.x; i < n_bones * 2u; i += 256u) sq[i] = b[i];
}

// bf_skin_vertices_kernel with the blend above: `bones` is [n_versions][n_bones][8], bone_stride = 8 n_bones.  A lane past the end
// holds index 0 and weight 0 and leaves at the barrier's far side; control flow is uniform up to it.
__global__ __launch_bounds__(256) void bf_skin_vertices_dq_kernel(const float *__restrict__ rest_pos, const float *__restrict__ rest_nrm,
                                                                  const uint4 *__restrict__ index, const float4 *__restrict__ weight, uint32_t nv,
                                                                  const float *__restrict__ bones, uint32_t n_bones, uint32_t bone_stride,
                                                                  float *__restrict__ pos, float *__restrict__ nrm, uint64_t vstride) {
    __shared__ float4 sq[256 * 2];
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, ver = blockIdx.y;
    const bool live = v < nv;
    uint4 ix = make_uint4(0u, 0u, 0u, 0u);
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    float x[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f};
    if (live) {
        ix = index[v];        // one 16-byte load each
        w = weight[v];
        for (int c = 0; c < 3; ++c) x[c] = rest_pos[3u * (size_t) v + c];
        if (rest_nrm)
            for (int c = 0; c < 3; ++c) n[c] = rest_nrm[3u * (size_t) v + c];
    }
    dq_table_load(sq, bones, n_bones, bone_stride, ver);
    __syncthreads();
    if (!live) return;
    const size_t o = (size_t) vstride * ver + 3u * (size_t) v;
    const DqBlend q = dq_blend(sq, ix, w);
    const float3 p = dq_point(q, x[0], x[1], x[2]);
    pos[o] = p.x, pos[o + 1] = p.y, pos[o + 2] = p.z;
    if (rest_nrm) {
        const float3 r = dq_rotate(q, n[0], n[1], n[2]);
        nrm[o] = r.x, nrm[o + 1] = r.y, nrm[o + 2] = r.z;
    }
}
BF_NS_END  // namespace bfd

// bfk_launch_skin_vertices for a shape in BF_SKIN_DUAL_QUATERNION: bones [n_versions][n_bones][8] (device, 16-byte aligned)
extern "C" hipError_t bfk_launch_skin_vertices_dq(const float *rest_pos, const float *rest_nrm, const uint4 *index, const float4 *weight,
                                                  uint32_t nv, const float *bones, uint32_t n_bones, float *pos, float *nrm,
                                                  uint32_t n_versions, hipStream_t stream) {
    if (nv == 0 || n_versions == 0) return hipSuccess;
    if (n_versions > 65535u || n_bones == 0 || n_bones > 256u || ((uintptr_t) bones & 15u)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bfd::bf_skin_vertices_dq_kernel, dim3((nv + 255u) / 256u, n_versions), dim3(256), 0, stream, rest_pos, rest_nrm, index,
                       weight, nv, bones, n_bones, n_bones * 8u, pos, nrm, (uint64_t) 3u * nv);
    return hipGetLastError();
}

BF_NS_BEGIN
// bf_scene_pose_morph / bf_render_morph_batch_device: morph targets (blend shapes) of one mesh shape, and the skin
// behind them in the same registers.  One thread per vertex, grid y = version: version v reads its n_targets weights `n_targets`
// floats further (and its bone table `bone_stride` floats further) and writes its vertices `vstride` floats further.
//   p = rest;  for k = 0 .. n_targets-1 in increasing k:  p_c = fl(p_c + fl(w_k d_k,c))    per coordinate, no FMA
//   n likewise from the rest normal and the normal deltas (dnrm == nullptr: the rest normal, bit for bit), not renormalised
//   SKIN: (p, n) then go through skin_blend (1, BF_SKIN_LINEAR) or dq_blend (2, BF_SKIN_DUAL_QUATERNION: the bone table is then
//   bf_skin_vertices_dq_kernel's) in place of the skin's own rest arrays; 0: no skin
// Every target is always evaluated: a zero weight takes no shortcut.  The deltas lie [target][vertex][3], so a wave's loads for one
// target are contiguous; the weights are indexed by blockIdx.y and the loop counter alone (uniform: scalar loads).  The target loop
// is unrolled four times to keep four targets' loads in flight; the sums are taken in increasing k all the same.  A lane past the
// end computes vertex nv - 1 again and stores nothing, so control flow is uniform up to the barrier.
template <int SKIN>
__global__ __launch_bounds__(256) void bf_morph_vertices_kernel(const float *__restrict__ rest_pos, const float *__restrict__ rest_nrm,
                                                                const float *__restrict__ dpos, const float *__restrict__ dnrm, uint32_t nv,
                                                                uint32_t n_targets, const float *__restrict__ wts,
                                                                const uint4 *__restrict__ index, const float4 *__restrict__ weight,
                                                                const float *__restrict__ bones, uint32_t n_bones, uint32_t bone_stride,
                                                                float *__restrict__ pos, float *__restrict__ nrm, uint64_t vstride) {
    __shared__ float4 sb4[SKIN == 1 ? 256 * 3 : (SKIN == 2 ? 256 * 2 : 1)];
    float *sb = reinterpret_cast<float *>(sb4);
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, ver = blockIdx.y;
    const bool live = v < nv;
    const size_t vc = 3u * (size_t) (live ? v : nv - 1u), tstride = 3u * (size_t) nv;
    uint4 ix = make_uint4(0u, 0u, 0u, 0u);
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (SKIN) {
        ix = index[vc / 3u];
        w = weight[vc / 3u];
        if (SKIN == 2) {
            dq_table_load(sb4, bones, n_bones, bone_stride, ver);
        } else {
            const float *b = bones + (size_t) bone_stride * ver;
            for (uint32_t i = threadIdx.x; i < n_bones * 12u; i += 256u) sb[i] = b[i];
        }
    }
    float x[3], n[3] = {0.f, 0.f, 0.f};
    for (int c = 0; c < 3; ++c) x[c] = rest_pos[vc + c];
    if (rest_nrm)
        for (int c = 0; c < 3; ++c) n[c] = rest_nrm[vc + c];
    const float *wv = wts + (size_t) n_targets * ver;
    const float *dp = dpos + vc, *dn = rest_nrm && dnrm ? dnrm + vc : nullptr;
    uint32_t k = 0;
    for (; k + 4u <= n_targets; k += 4u) {
        float d[4][3], e[4][3];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            for (int c = 0; c < 3; ++c) d[j][c] = dp[(size_t) (k + j) * tstride + c];
        if (dn) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                for (int c = 0; c < 3; ++c) e[j][c] = dn[(size_t) (k + j) * tstride + c];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float wk = wv[k + j];
            for (int c = 0; c < 3; ++c) x[c] = __fadd_rn(x[c], __fmul_rn(wk, d[j][c]));
            if (dn)
                for (int c = 0; c < 3; ++c) n[c] = __fadd_rn(n[c], __fmul_rn(wk, e[j][c]));
        }
    }
    for (; k < n_targets; ++k) {
        const float wk = wv[k];
        for (int c = 0; c < 3; ++c) x[c] = __fadd_rn(x[c], __fmul_rn(wk, dp[(size_t) k * tstride + c]));
        if (dn)
            for (int c = 0; c < 3; ++c) n[c] = __fadd_rn(n[c], __fmul_rn(wk, dn[(size_t) k * tstride + c]));
    }
    if (SKIN) __syncthreads();
    if (!live) return;
    const size_t o = (size_t) vstride * ver + vc;
    if (SKIN == 2) {
        const DqBlend q = dq_blend(sb4, ix, w);
        const float3 p = dq_point(q, x[0], x[1], x[2]);
        pos[o] = p.x, pos[o + 1] = p.y, pos[o + 2] = p.z;
        if (rest_nrm) {
            const float3 r = dq_rotate(q, n[0], n[1], n[2]);
            nrm[o] = r.x, nrm[o + 1] = r.y, nrm[o + 2] = r.z;
        }
    } else if (SKIN == 1) {
        const float3 p = skin_blend(sb, ix, w, x[0], x[1], x[2], true);
        pos[o] = p.x, pos[o + 1] = p.y, pos[o + 2] = p.z;
        if (rest_nrm) {
            const float3 r = skin_blend(sb, ix, w, n[0], n[1], n[2], false);
            nrm[o] = r.x, nrm[o + 1] = r.y, nrm[o + 2] = r.z;
        }
    } else {
        pos[o] = x[0], pos[o + 1] = x[1], pos[o + 2] = x[2];
        if (rest_nrm) nrm[o] = n[0], nrm[o + 1] = n[1], nrm[o + 2] = n[2];
    }
}
BF_NS_END  // namespace bfd

// n_versions poses of one morphed shape: weights [n_versions][n_targets] (device) -> pos (and nrm, if rest_nrm is given),
// [n_versions][nv][3] each.  bones != nullptr ([n_versions][n_bones][12], device; dq: [n_versions][n_bones][8], 16-byte aligned, the
// shape is in BF_SKIN_DUAL_QUATERNION): skinned behind the morph, with `index` and `weight`
extern "C" hipError_t bfk_launch_morph_vertices(const float *rest_pos, const float *rest_nrm, const float *dpos, const float *dnrm, uint32_t nv,
                                                uint32_t n_targets, const float *wts, const uint4 *index, const float4 *weight,
                                                const float *bones, uint32_t n_bones, int dq, float *pos, float *nrm, uint32_t n_versions,
                                                hipStream_t stream) {
    if (nv == 0 || n_versions == 0) return hipSuccess;
    if (n_versions > 65535u || n_targets == 0 || n_targets > 256u) return hipErrorInvalidValue;
    const dim3 grid((nv + 255u) / 256u, n_versions);
    if (bones) {
        if (n_bones == 0 || n_bones > 256u || !index || !weight) return hipErrorInvalidValue;
        if (dq && ((uintptr_t) bones & 15u)) return hipErrorInvalidValue;
        if (dq)
            hipLaunchKernelGGL(bfd::bf_morph_vertices_kernel<2>, grid, dim3(256), 0, stream, rest_pos, rest_nrm, dpos, dnrm, nv, n_targets, wts, index,
                               weight, bones, n_bones, n_bones * 8u, pos, nrm, (uint64_t) 3u * nv);
        else
            hipLaunchKernelGGL(bfd::bf_morph_vertices_kernel<1>, grid, dim3(256), 0, stream, rest_pos, rest_nrm, dpos, dnrm, nv, n_targets, wts, index,
                               weight, bones, n_bones, n_bones * 12u, pos, nrm, (uint64_t) 3u * nv);
    } else {
        hipLaunchKernelGGL(bfd::bf_morph_vertices_kernel<0>, grid, dim3(256), 0, stream, rest_pos, rest_nrm, dpos, dnrm, nv, n_targets, wts, index,
                           weight, bones, 0u, 0u, pos, nrm, (uint64_t) 3u * nv);
    }
    return hipGetLastError();
}

BF_NS_BEGIN
// Recomputed vertex normals (BF_NORMALS_RECOMPUTE, bf_vertex_normals): angle-weighted face normals summed per vertex.
// The arithmetic is stated ONCE, here, for the kernel and for the host entry alike: fp32, every product, sum, difference, quotient
// and square root rounded (IEEE division and square root), no FMA outside bf_acos.  The device spells the operations __fmul_rn /
// __fadd_rn / ..., the host as plain operators of this object (compiled with -ffp-contract=off).  For face (p0, p1, p2):
//   n  = cross(p1 - p0, p2 - p0), each component fl(fl(a b) - fl(c d));  l2 = fl(fl(fl(nx^2) + fl(ny^2)) + fl(nz^2))
//   the face contributes nothing unless l2 > 0;  nh = n / sqrt(l2) per component
//   corner j: a = p[j+1] - p[j], b = p[j+2] - p[j], la = sqrt(dot(a, a)), lb likewise (dot = (x + y) + z of the rounded products);
//     the corner contributes nothing unless la > 0 and lb > 0 (an edge whose squared length underflows to zero while l2 > 0);
//     c = dot(a / la, b / lb) clamped to [-1, 1] by comparisons (a NaN stays one), theta = bf_acos(c), contribution fl(nh theta)
// and per vertex: s = +0, plus its contributions in increasing face index, one add per component each; len = sqrt(dot(s, s));
// s / len if len != 0, else (1, 0, 0).
BF_HD float vn_mul(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fmul_rn(a, b);
#else
    return a * b;
#endif
}
BF_HD float vn_add(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(a, b);
#else
    return a + b;
#endif
}
BF_HD float vn_sub(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fsub_rn(a, b);
#else
    return a - b;
#endif
}
BF_HD float vn_div(float a, float b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn(a, b);
#else
    return a / b;
#endif
}
// (not __fsqrt_rn: HIP defines it as the NATIVE square root, v_sqrt_f32's 1 ulp, unless OCML_BASIC_ROUNDED_OPERATIONS is set; the
// builtin is the correctly rounded one in this object, as in bf_acos, and sqrtss on the host)
BF_HD float vn_sqrt(float a) { return __builtin_sqrtf(a); }
BF_HD float vn_acos(float c) {
#if defined(__HIP_DEVICE_COMPILE__)
    return acos_cr(c);
#else
    return bf_acos(c);
#endif
}
BF_HD float vn_dot(const float *a, const float *b) { return vn_add(vn_add(vn_mul(a[0], b[0]), vn_mul(a[1], b[1])), vn_mul(a[2], b[2])); }

// what face (p0, p1, p2) contributes to its corner j; false: nothing
BF_HD bool vn_corner(const float *p0, const float *p1, const float *p2, uint32_t j, float out[3]) {
    float e1[3], e2[3], n[3], a[3], b[3];
    for (int c = 0; c < 3; ++c) e1[c] = vn_sub(p1[c], p0[c]), e2[c] = vn_sub(p2[c], p0[c]);
    n[0] = vn_sub(vn_mul(e1[1], e2[2]), vn_mul(e1[2], e2[1]));
    n[1] = vn_sub(vn_mul(e1[2], e2[0]), vn_mul(e1[0], e2[2]));
    n[2] = vn_sub(vn_mul(e1[0], e2[1]), vn_mul(e1[1], e2[0]));
    const float l2 = vn_dot(n, n);
    if (!(l2 > 0.f)) return false;
    const float l = vn_sqrt(l2);
    const float *q = j == 0u ? p0 : (j == 1u ? p1 : p2), *qa = j == 0u ? p1 : (j == 1u ? p2 : p0), *qb = j == 0u ? p2 : (j == 1u ? p0 : p1);
    for (int c = 0; c < 3; ++c) a[c] = vn_sub(qa[c], q[c]), b[c] = vn_sub(qb[c], q[c]);
    const float la = vn_sqrt(vn_dot(a, a)), lb = vn_sqrt(vn_dot(b, b));
    if (!(la > 0.f) || !(lb > 0.f)) return false;
    for (int c = 0; c < 3; ++c) a[c] = vn_div(a[c], la), b[c] = vn_div(b[c], lb);
    const float d = vn_dot(a, b);
    const float theta = vn_acos(d < -1.f ? -1.f : (d > 1.f ? 1.f : d));
    for (int c = 0; c < 3; ++c) out[c] = vn_mul(vn_div(n[c], l), theta);
    return true;
}
BF_HD void vn_finish(const float s[3], float out[3]) {
    const float len = vn_sqrt(vn_dot(s, s));
    if (len != 0.f) {
        for (int c = 0; c < 3; ++c) out[c] = vn_div(s[c], len);
    } else {
        out[0] = 1.f, out[1] = 0.f, out[2] = 0.f;
    }
}

// One lane per vertex, grid y = geometry version (version v reads and writes `vstride` floats further, as bf_skin_vertices_kernel).
// offset[nv + 1] / entries: the inverted index of the shape's faces (bf_mesh.cpp: normal_index), one uint4 per incident corner, sorted
// by face: the face's three vertex indices in the order the scene gave them (each < nv, checked where the index is built), then the
// corner number.  The lane recomputes every incident face's normal and its own corner's angle from the version's positions and sums
// in list order: no atomics (their arrival order would make the sum irreproducible), no LDS.  The next entry's positions (and the
// entry behind it) are loaded before the arithmetic of the current one.  A vertex of very high valence makes its lane loop that
// long while the rest of its wave waits: correct, not fast.
__global__ __launch_bounds__(256) void bf_vertex_normals_kernel(const uint32_t *__restrict__ offset, const uint4 *__restrict__ entries, uint32_t nv,
                                                                const float *__restrict__ pos, float *__restrict__ nrm, uint64_t vstride) {
    const uint32_t v = blockIdx.x * 256u + threadIdx.x;
    if (v >= nv) return;
    const float *p = pos + vstride * blockIdx.y;
    uint32_t k = offset[v];
    const uint32_t end = offset[v + 1u];
    float s[3] = {0.f, 0.f, 0.f}, g[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint4 e = make_uint4(0u, 0u, 0u, 0u), e_next = e;
    if (k < end) {
        e = entries[k];
        if (k + 1u < end) e_next = entries[k + 1u];
        const float *p0 = p + 3u * (size_t) e.x, *p1 = p + 3u * (size_t) e.y, *p2 = p + 3u * (size_t) e.z;
        for (int c = 0; c < 3; ++c) g[c] = p0[c], g[3 + c] = p1[c], g[6 + c] = p2[c];
    }
    for (; k < end; ++k) {
        float cur[9];
        for (int c = 0; c < 9; ++c) cur[c] = g[c];
        const uint32_t j = e.w;
        if (k + 1u < end) {
            e = e_next;
            const float *p0 = p + 3u * (size_t) e.x, *p1 = p + 3u * (size_t) e.y, *p2 = p + 3u * (size_t) e.z;
            for (int c = 0; c < 3; ++c) g[c] = p0[c], g[3 + c] = p1[c], g[6 + c] = p2[c];
            if (k + 2u < end) e_next = entries[k + 2u];
        }
        float t[3];
        if (vn_corner(cur, cur + 3, cur + 6, j, t))
            for (int c = 0; c < 3; ++c) s[c] = vn_add(s[c], t[c]);
    }
    float r[3];
    vn_finish(s, r);
    float *o = nrm + vstride * blockIdx.y + 3u * (size_t) v;
    o[0] = r[0], o[1] = r[1], o[2] = r[2];
}
BF_NS_END  // namespace bfd

// n_versions position arrays [n_versions][nv][3] (device) of one shape -> its vertex normals, the same layout
extern "C" hipError_t bfk_launch_vertex_normals(const uint32_t *offset, const uint4 *entries, uint32_t nv, const float *pos, float *nrm,
                                                uint32_t n_versions, hipStream_t stream) {
    if (nv == 0 || n_versions == 0) return hipSuccess;
    if (n_versions > 65535u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bfd::bf_vertex_normals_kernel, dim3((nv + 255u) / 256u, n_versions), dim3(256), 0, stream, offset, entries, nv, pos, nrm,
                       (uint64_t) 3u * nv);
    return hipGetLastError();
}

/* bf_vertex_normals (bf_mesh.cpp checks the arguments): the statement above on the host, faces in order, no device. */
extern "C" void bfk_host_vertex_normals(uint32_t nv, const float *pos, uint32_t nf, const uint32_t *idx, float *out) {
    for (size_t i = 0; i < 3 * (size_t) nv; ++i) out[i] = 0.f;
    for (uint32_t f = 0; f < nf; ++f) {
        const uint32_t *ix = idx + 3 * (size_t) f;
        for (uint32_t j = 0; j < 3u; ++j) {
            float t[3];
            if (!bfd::vn_corner(pos + 3 * (size_t) ix[0], pos + 3 * (size_t) ix[1], pos + 3 * (size_t) ix[2], j, t)) continue;
            float *s = out + 3 * (size_t) ix[j];
            for (int c = 0; c < 3; ++c) s[c] = bfd::vn_add(s[c], t[c]);
        }
    }
    for (uint32_t v = 0; v < nv; ++v) {
        const float s[3] = {out[3 * (size_t) v], out[3 * (size_t) v + 1], out[3 * (size_t) v + 2]};
        bfd::vn_finish(s, out + 3 * (size_t) v);
    }
}
