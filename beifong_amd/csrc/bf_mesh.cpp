// "The meshes of this handle have moved" (DESIGN.md 6d): translations, rigid transforms, vertex updates, the rebuild of both trees
// and the batches with a geometry version per render.  State: bf_scene::mesh (bf_scene.h); kernels: bf_geom.hip, bf_build.hip.
// Skins and morph targets, which end in a vertex update or a deform batch of this file: bf_pose.cpp.
#include "bf_scene.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

namespace {

int g_rebuild_fail_alloc = 0;      // test hook: the n-th allocation of the rebuild's swap phase fails

// The one way this file allocates device memory: `bytes` (0: none, *out = nullptr) pushed onto `list`; BF_ERR_NOMEM names `who`.
// fail_at: the rebuild's test hook (the fail_at-th allocation through this object fails).
struct DevAlloc {
    std::vector<void *> &list;
    const char *who;
    int fail_at = 0, n = 0;
    template <class T> bf_status operator()(size_t bytes, T **out) {
        *out = nullptr;
        if (!bytes) return BF_OK;
        void *q = nullptr;
        const bool inject = fail_at && ++n == fail_at;
        const hipError_t he = inject ? hipErrorOutOfMemory : hipMalloc(&q, bytes);
        if (he != hipSuccess) {
            (void) hipGetLastError();
            return fail(BF_ERR_NOMEM, "%s: hipMalloc(%zu bytes): %s", who, bytes, hipGetErrorString(he));
        }
        list.push_back(q);
        *out = (T *) q;
        return BF_OK;
    }
};

// n entries of a [..][12] transform table as the 16-float records bfk_launch_rigid reads: word 12 = the shape moves, 13..15 = 0
void pack_rigid(float *out, const float *to_world, const uint8_t *moves, size_t n) {
    for (size_t r = 0; r < n; ++r) {
        float *o = out + 16 * r;
        std::memcpy(o, to_world + 12 * r, 12 * sizeof(float));
        o[12] = moves[r] ? 1.f : 0.f;
        o[13] = o[14] = o[15] = 0.f;
    }
}

// The bound on ray origins the boxes must be padded for once the meshes stand at `xf` (a [3][4] matrix every `stride` floats): `oscale`
// raised to cover each mesh's base box through |R| plus |t|, with a little margin.  moves: the moved shapes only (a transform call:
// unmoved meshes stay under the bound they had); nullptr: every shape (a pose after a vertex update covers unmoved shapes' new boxes too).
float origin_bound(const std::vector<float> &mesh_box, uint32_t n_shapes, const float *xf, size_t stride, const uint8_t *moves, float oscale) {
    for (uint32_t k = 0; k < n_shapes; ++k) {
        const float *b = &mesh_box[6 * (size_t) k], *m = xf + stride * k;
        if ((moves && !moves[k]) || !(b[0] <= b[3])) continue;
        for (int r = 0; r < 3; ++r) {
            double v = std::fabs((double) m[4 * r + 3]);
            for (int c = 0; c < 3; ++c) v += std::fabs((double) m[4 * r + c]) * std::max(std::fabs((double) b[c]), std::fabs((double) b[3 + c]));
            oscale = std::max(oscale, (float) (v * (1.0 + 1e-5)));
        }
    }
    return oscale;
}

// Layout of one geometry version of a batch, in float4 rows from its start: triangles (+ the kTriPad rows behind them), vertex
// normals, four-wide nodes, sixteen-wide nodes, quantised nodes, then the refit's scratch (unpadded child bounds of both trees).
// with_vel: the velocity rows of the version too (bf_velocity.h; three per triangle slot), last, so that the other arrays lie where
// they lie without them
struct MotionLayout { size_t tris = 0, normals = 0, nodes = 0, wnodes = 0, qnodes = 0, ubox4 = 0, ubox16 = 0, vel = 0, rows = 0; };
MotionLayout motion_layout(const bfd::DScene &d, bool with_vel) {
    MotionLayout L;
    size_t r = 0;
    auto take = [&](size_t &at, size_t rows) {
        at = r;
        r += (rows + 7) & ~size_t(7);      // every array on a 128-byte line
    };
    take(L.tris, (size_t) d.n_tris * bfd::kTriStride + kTriPad);
    take(L.normals, d.normals ? (size_t) d.n_tris * 3 : 0);
    take(L.nodes, (size_t) d.n_nodes * 8);
    take(L.wnodes, d.wnodes ? (size_t) d.n_wnodes * 32 : 0);
    take(L.qnodes, d.qnodes ? (size_t) d.n_nodes * 4 : 0);
    take(L.ubox4, (size_t) d.n_nodes * 8);
    take(L.ubox16, d.wnodes ? (size_t) d.n_wnodes * 32 : 0);
    take(L.vel, with_vel ? (size_t) d.n_tris * bfvel::kRowsPerSlot : 0);
    L.rows = r;
    return L;
}

// where one pass of the refit kernels writes: the handle's own arrays (run_pose), or the versions of a batch chunk in the arena
struct RefitDst {
    float4 *tris, *normals, *nodes, *wnodes, *qnodes, *ubox4, *ubox16;
    uint32_t n_versions;
    uint64_t vstride;      // float4 rows between versions
};
RefitDst arena_dst(const bf_scene *scene, float4 *a, const MotionLayout &L, uint32_t n_versions) {
    const bfd::DScene &d = scene->d;
    return {a + L.tris, d.normals ? a + L.normals : nullptr, a + L.nodes, d.wnodes ? a + L.wnodes : nullptr, d.qnodes ? a + L.qnodes : nullptr,
            a + L.ubox4, a + L.ubox16, n_versions, L.rows};
}
// the base rows through the tables `xf` (xf_stride floats between versions) into `o`, both trees re-fitted; nrm0: the base normals to
// turn along (nullptr: `o`'s normals are left alone)
hipError_t launch_rigid(const bf_scene *scene, const float4 *nrm0, const float *xf, uint32_t xf_stride, float oscale, const RefitDst &o,
                        hipStream_t stream) {
    const bfd::DScene &d = scene->d;
    const MeshState::Refit &rf = scene->mesh.refit;
    const MeshState::Base b = scene->mesh.base(d);
    return bfk_launch_rigid(b.tris, o.tris, nrm0, nrm0 ? o.normals : nullptr, d.n_tris, xf, b.nodes, o.nodes, o.qnodes, d.n_nodes, rf.lvl4, rf.off4.data(),
                            (uint32_t) rf.off4.size() - 1u, o.ubox4, b.wnodes, o.wnodes, rf.lvl16, rf.off16.data(), (uint32_t) rf.off16.size() - 1u,
                            o.ubox16, 2e-7f * oscale, o.n_versions, o.vstride, xf_stride, stream);
}
// both trees of `o` re-fitted to the triangle rows `o` holds already
hipError_t launch_refit(const bf_scene *scene, float oscale, const RefitDst &o, hipStream_t stream) {
    const bfd::DScene &d = scene->d;
    const MeshState::Refit &rf = scene->mesh.refit;
    const MeshState::Base b = scene->mesh.base(d);
    return bfk_launch_refit(o.tris, b.nodes, o.nodes, o.qnodes, d.n_nodes, rf.lvl4, rf.off4.data(), (uint32_t) rf.off4.size() - 1u, o.ubox4, b.wnodes,
                            o.wnodes, rf.lvl16, rf.off16.data(), (uint32_t) rf.off16.size() - 1u, o.ubox16, 2e-7f * oscale, o.n_versions, o.vstride,
                            stream);
}

// The geometry a handle moves: d.tris / d.nodes / d.wnodes / d.qnodes writable by this handle, the base rows kept in tris0 / nodes0 / wnodes0.
bf_status own_geometry(bf_scene *scene, hipStream_t stream, const char *who) {
    MeshState &m = scene->mesh;
    bfd::DScene &d = scene->d;
    const MeshState::Bytes B = MeshState::bytes(d);
    const bool shared = scene->geom_token.use_count() > 1 && !m.geom_private;
    if (!shared && m.tris0) return BF_OK;
    // shared with clones: copy on write, this handle gets its own moved copies (quantised nodes too: re-quantised by the caller's
    // kernels).  Else, first use: a copy of the geometry as created, so that every later offset is applied to it (no drift).
    const size_t bytes[4] = {B.tris, B.nodes, B.wnodes, shared && d.qnodes ? B.nodes / 2 : 0};
    // all or nothing: the handle's pointers change only once every copy exists (never tris0 set and nodes0 null for the next call)
    std::vector<void *> got;
    DevAlloc take{got, who};
    float4 *p[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < 4; ++k) {
        const bf_status st = take(bytes[k], &p[k]);
        if (st != BF_OK) {
            for (void *q : got) (void) hipFree(q);
            return st;
        }
    }
    for (void *q : got) scene->owned.push_back(q);
    if (shared) {
        // the base is the geometry as created if this handle has it (it translated in place before it was cloned), else the shared arrays
        if (!m.tris0) {
            m.tris0 = const_cast<float4 *>(d.tris);
            m.nodes0 = const_cast<float4 *>(d.nodes);
            m.wnodes0 = const_cast<float4 *>(d.wnodes);
            m.base_private = false;
        }
        d.tris = p[0];
        d.nodes = p[1];
        d.wnodes = p[2];
        if (d.qnodes) d.qnodes = p[3];
        m.geom_private = true;       // (the token stays shared: tris0 / nodes0 may still READ the shared arrays)
    } else {
        HIP_TRY(hipMemcpyAsync(p[0], d.tris, B.tris, hipMemcpyDeviceToDevice, stream));
        if (B.nodes) HIP_TRY(hipMemcpyAsync(p[1], d.nodes, B.nodes, hipMemcpyDeviceToDevice, stream));
        if (B.wnodes) HIP_TRY(hipMemcpyAsync(p[2], d.wnodes, B.wnodes, hipMemcpyDeviceToDevice, stream));
        m.tris0 = p[0];
        m.nodes0 = p[1];
        m.wnodes0 = p[2];
        m.base_private = true;
    }
    return BF_OK;
}

// First transform of a handle: the level lists of both trees (from the base nodes' child references, read back once), the unpadded-bound
// scratch, the device transform table and every mesh's base box (read back once).  Runs before own_geometry: a failure changes no array.
bf_status refit_prepare(bf_scene *scene, hipStream_t stream) {
    MeshState::Refit &rf = scene->mesh.refit;
    const bfd::DScene &d = scene->d;
    HIP_TRY(hipStreamSynchronize(stream));      // the rows may still be written by work enqueued on `stream`
    const MeshState::Base base = scene->mesh.base(d);
    // levels by breadth-first order from the root: children reference deeper nodes only
    auto levels = [](const std::vector<int32_t> &refs, uint32_t width, int32_t root, std::vector<uint32_t> &off, std::vector<uint32_t> &flat) {
        off.assign(1, 0u);
        flat.clear();
        if (root < 0) return;
        flat.push_back((uint32_t) root);
        for (size_t begin = 0; begin < flat.size();) {
            const size_t end = flat.size();
            off.push_back((uint32_t) end);
            for (size_t i = begin; i < end; ++i)
                for (uint32_t k = 0; k < width; ++k) {
                    const int32_t r = refs[(size_t) flat[i] * width + k];
                    if (r >= 0) flat.push_back((uint32_t) r);
                }
            begin = end;
        }
    };
    DevAlloc take{scene->owned, "refit_prepare"};
    auto upload_levels = [&](const std::vector<uint32_t> &v, uint32_t **out) -> bf_status {
        const bf_status ast = take(v.size() * sizeof(uint32_t), out);
        if (ast != BF_OK || v.empty()) return ast;
        HIP_TRY(hipMemcpy(*out, v.data(), v.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        return BF_OK;
    };
    bf_status st;
    std::vector<uint32_t> flat;
    if (d.n_nodes) {
        std::vector<int32_t> refs((size_t) d.n_nodes * 4);       // row 6 of every Node4
        HIP_TRY(hipMemcpy2D(refs.data(), 16, (const char *) base.nodes + 6 * sizeof(float4), 8 * sizeof(float4), 16, d.n_nodes, hipMemcpyDeviceToHost));
        levels(refs, 4, d.root, rf.off4, flat);
        if ((st = upload_levels(flat, &rf.lvl4)) != BF_OK) return st;
        if ((st = take((size_t) d.n_nodes * 8 * sizeof(float4), &rf.ubox4)) != BF_OK) return st;
    } else {
        rf.off4.assign(1, 0u);
    }
    if (d.wnodes && d.n_wnodes) {
        std::vector<int32_t> refs((size_t) d.n_wnodes * 16);     // word 6 of every Node16 child record
        HIP_TRY(hipMemcpy2D(refs.data(), 4, (const char *) base.wnodes + 6 * sizeof(float), 8 * sizeof(float), 4, refs.size(), hipMemcpyDeviceToHost));
        levels(refs, 16, d.wroot, rf.off16, flat);
        if ((st = upload_levels(flat, &rf.lvl16)) != BF_OK) return st;
        if ((st = take((size_t) d.n_wnodes * 32 * sizeof(float4), &rf.ubox16)) != BF_OK) return st;
    } else {
        rf.off16.assign(1, 0u);
    }
    if (rf.have_boxes) {
        rf.ready = true;
        return BF_OK;
    }
    if ((st = take((size_t) scene->info.n_shapes * 16 * sizeof(float), &rf.xf)) != BF_OK) return st;
    std::vector<float4> tris((size_t) d.n_tris * bfd::kTriStride);
    HIP_TRY(hipMemcpy(tris.data(), base.tris, tris.size() * sizeof(float4), hipMemcpyDeviceToHost));
    const float inf = std::numeric_limits<float>::infinity();
    rf.mesh_box.assign((size_t) scene->info.n_shapes * 6, 0.f);
    for (uint32_t k = 0; k < scene->info.n_shapes; ++k)
        for (int a = 0; a < 3; ++a) rf.mesh_box[6 * k + a] = inf, rf.mesh_box[6 * k + 3 + a] = -inf;
    for (size_t t = 0; t < d.n_tris; ++t) {
        const float4 *r = &tris[t * bfd::kTriStride];
        uint32_t shape;
        std::memcpy(&shape, &r[1].w, 4);
        float *b = &rf.mesh_box[6 * (size_t) shape];
        for (int j = 0; j < 3; ++j) {
            const float p[3] = {r[j].x, r[j].y, r[j].z};
            for (int a = 0; a < 3; ++a) b[a] = std::min(b[a], p[a]), b[3 + a] = std::max(b[3 + a], p[a]);
        }
    }
    rf.have_boxes = true;
    rf.ready = true;
    return BF_OK;
}

// The checks of one transform table ([n_shapes][12], bf_scene_transform_meshes' rules): moves[k] = 1 if shape k's entry is not
// exactly the identity.  `who` names the call (and the render, for a batch) in the error text, which also names the shape.
bf_status check_rigid_table(const bf_scene *scene, uint32_t n_shapes, const float *to_world, const char *who, uint8_t *moves) {
    for (uint32_t k = 0; k < n_shapes; ++k) {
        const float *m = to_world + 12 * (size_t) k;
        moves[k] = 0;
        for (int j = 0; j < 12; ++j)
            if (!std::isfinite(m[j])) return fail(BF_ERR_INVALID, "%s shape %u: non-finite entry", who, k);
        for (int j = 0; j < 12; ++j) moves[k] |= m[j] != ((j % 5 == 0) ? 1.f : 0.f);
        if (!moves[k]) continue;
        double e = 0.0;
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                double d = a == b ? -1.0 : 0.0;
                for (int r = 0; r < 3; ++r) d += (double) m[4 * r + a] * (double) m[4 * r + b];
                e = std::max(e, std::fabs(d));
            }
        const double det = (double) m[0] * ((double) m[5] * m[10] - (double) m[6] * m[9]) - (double) m[1] * ((double) m[4] * m[10] - (double) m[6] * m[8]) +
                           (double) m[2] * ((double) m[4] * m[9] - (double) m[5] * m[8]);
        if (!(e <= 1e-5) || !(det > 0.0))
            return fail(BF_ERR_INVALID, "%s shape %u: not a rigid motion (|R^T R - I| = %g, det R = %g)", who, k, e, det);
        const bfd::DShape &sh = scene->ends.shapes_host[k];
        if (sh.type != BF_SHAPE_MESH)
            return fail(BF_ERR_INVALID, "%s shape %u is not a mesh: its entry must be the identity", who, k);
        if (sh.emitter >= 0)
            return fail(BF_ERR_UNSUPPORTED, "%s mesh shape %u carries emitter %d (its sampling tables are built "
                                            "from the triangles as created); create a new scene", who, k, sh.emitter);
    }
    return BF_OK;
}

// The pose table (pose_kind / pose_xf) over the base rows into the arrays the handle renders; a translation leaves the base normals as they are.
bf_status run_pose(bf_scene *scene, hipStream_t stream) {
    MeshState &m = scene->mesh;
    const size_t bytes = m.pose_xf.size() * sizeof(float);
    bf_scene::Stage *stg = nullptr;
    bf_status st = stage_acquire(scene, bytes, &stg);
    if (st != BF_OK) return st;
    std::memcpy(stg->host, m.pose_xf.data(), bytes);
    HIP_TRY(hipMemcpyAsync(m.refit.xf, stg->host, bytes, hipMemcpyHostToDevice, stream));
    if ((st = stage_release_after(stg, stream)) != BF_OK) return st;
    const bool turn_normals = m.pose_kind != 1 && m.normals0 != nullptr;
    if (!turn_normals && m.normals0)
        HIP_TRY(hipMemcpyAsync(const_cast<float4 *>(scene->d.normals), m.normals0, MeshState::bytes(scene->d).normals, hipMemcpyDeviceToDevice, stream));
    const bfd::DScene &d = scene->d;
    const RefitDst own = {const_cast<float4 *>(d.tris), const_cast<float4 *>(d.normals), const_cast<float4 *>(d.nodes), const_cast<float4 *>(d.wnodes),
                          const_cast<float4 *>(d.qnodes), m.refit.ubox4, m.refit.ubox16, 1u, 0u};
    HIP_TRY(launch_rigid(scene, turn_normals ? m.normals0 : nullptr, m.refit.xf, 0u, m.origin_scale_built, own, stream));
    m.normals_moved = m.pose_kind == 2 && scene->d.normals != nullptr;
    return BF_OK;
}
// The handle's latest pose again, after its base rows or boxes have changed (a vertex update; a translation of deformed meshes).
bf_status apply_pose(bf_scene *scene, hipStream_t stream) {
    MeshState &m = scene->mesh;
    const uint32_t n_shapes = scene->info.n_shapes;
    if (m.pose_xf.size() != (size_t) n_shapes * 16) {
        m.pose_xf.assign((size_t) n_shapes * 16, 0.f);
        for (uint32_t k = 0; k < n_shapes; ++k) m.pose_xf[16 * (size_t) k] = m.pose_xf[16 * (size_t) k + 5] = m.pose_xf[16 * (size_t) k + 10] = 1.f;
    }
    // ray origins lie on the posed meshes: raise (never lower) the padding bound over EVERY shape, unmoved ones with a new box included
    m.origin_scale_built = origin_bound(m.refit.mesh_box, n_shapes, m.pose_xf.data(), 16, nullptr, m.origin_scale_built);
    return run_pose(scene, stream);
}

// The corner table (shared with clones; built once from the scene's indices and the rows' prim / shape words) and the violation counter.
bf_status deform_prepare(bf_scene *scene, hipStream_t stream) {
    bf_geometry &g = *scene->geom;
    MeshState &m = scene->mesh;
    if (!g.corners) {
        HIP_TRY(hipStreamSynchronize(stream));
        const float4 *rows = m.base(scene->d).tris;
        std::vector<uint32_t> w((size_t) scene->d.n_tris * bfd::kTriStride);       // the .w words: prim, shape, tag per slot
        HIP_TRY(hipMemcpy2D(w.data(), 4, (const char *) rows + 12, sizeof(float4), 4, w.size(), hipMemcpyDeviceToHost));
        std::vector<uint4> corners(scene->d.n_tris);
        for (size_t t = 0; t < corners.size(); ++t) {
            const uint32_t prim = w[3 * t], shape = w[3 * t + 1];
            if (shape >= g.topo.size() || prim < g.topo[shape].prim0 || prim - g.topo[shape].prim0 >= g.topo[shape].n_faces)
                return fail(BF_ERR_DEVICE, "bf_scene_update_vertices: triangle slot %zu names primitive %u of shape %u, which the scene "
                                           "description does not have", t, prim, shape);
            const uint32_t *ix = &g.topo[shape].indices[3 * (size_t) (prim - g.topo[shape].prim0)];
            corners[t] = make_uint4(ix[0], ix[1], ix[2], shape);
        }
        uint4 *q = nullptr;
        const bf_status st = DevAlloc{g.owned, "bf_scene_update_vertices"}(corners.size() * sizeof(uint4), &q);
        if (st != BF_OK) return st;
        HIP_TRY(hipMemcpy(q, corners.data(), corners.size() * sizeof(uint4), hipMemcpyHostToDevice));
        g.corners = q;
        // the table holds them now; a mesh with vertex normals keeps its own (normal_index builds the inverted index from them)
        for (bf_geometry::MeshTopo &tp : g.topo)
            if (!tp.has_normals) std::vector<uint32_t>().swap(tp.indices);
    }
    if (!m.bad) {
        HIP_TRY(hipMalloc((void **) &m.bad, 2 * sizeof(uint32_t)));
        HIP_TRY(hipMemset(m.bad, 0, 2 * sizeof(uint32_t)));
        HIP_TRY(hipHostMalloc((void **) &m.bad_host, 2 * sizeof(uint32_t)));
        m.bad_host[0] = m.bad_host[1] = 0u;
        HIP_TRY(hipEventCreateWithFlags(&m.bad_ev, hipEventDisableTiming));
    }
    return BF_OK;
}

// Behind every gather of a device form: the counter on its way to the host, where deform_report() turns a non-zero count into an error.
bf_status deform_watch(bf_scene *scene, hipStream_t stream) {
    MeshState &m = scene->mesh;
    HIP_TRY(hipMemcpyAsync(m.bad_host, m.bad, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(m.bad_ev, stream));
    m.bad_pending = true;
    return BF_OK;
}

// ---- recomputed normals (bf_scene_set_normal_mode) ---------------------------------------------------------------------
// The inverted index of shape `shape` (bf_scene.h: NormalIndex), built from the indices the scene was created with at the first use
// by any handle that shares the geometry: per vertex its incident corners, faces in increasing order — the order of the sum.
bf_status normal_index(bf_scene *scene, uint32_t shape, const char *who, const bf_geometry::NormalIndex **out) {
    bf_geometry &g = *scene->geom;
    if (g.normal_index.size() < g.topo.size()) g.normal_index.resize(g.topo.size());
    if (!g.normal_index[shape]) {
        const bf_geometry::MeshTopo &tp = g.topo[shape];
        const uint32_t nv = tp.n_vertices;
        const size_t n_corners = 3 * (size_t) tp.n_faces;
        if (tp.indices.size() != n_corners)
            return fail(BF_ERR_DEVICE, "%s shape %u: the scene no longer holds the indices of this mesh", who, shape);
        if (n_corners > UINT32_MAX) return fail(BF_ERR_UNSUPPORTED, "%s shape %u: %zu corners (at most 2^32 - 1)", who, shape, n_corners);
        std::vector<uint32_t> off((size_t) nv + 1, 0u);
        for (size_t i = 0; i < n_corners; ++i) {
            if (tp.indices[i] >= nv) return fail(BF_ERR_INVALID, "%s shape %u: face %zu names vertex %u of %u", who, shape, i / 3, tp.indices[i], nv);
            ++off[(size_t) tp.indices[i] + 1];
        }
        for (uint32_t v = 0; v < nv; ++v) off[(size_t) v + 1] += off[v];
        std::vector<uint32_t> at(off.begin(), off.end() - 1);
        std::vector<uint4> ent(n_corners);
        for (uint32_t f = 0; f < tp.n_faces; ++f) {
            const uint32_t *ix = &tp.indices[3 * (size_t) f];
            for (uint32_t j = 0; j < 3u; ++j) ent[at[ix[j]]++] = make_uint4(ix[0], ix[1], ix[2], j);
        }
        auto idx = std::make_shared<bf_geometry::NormalIndex>();
        hipError_t he = hipMalloc((void **) &idx->offset, off.size() * sizeof(uint32_t));
        if (he == hipSuccess && n_corners) he = hipMalloc((void **) &idx->entries, n_corners * sizeof(uint4));
        if (he != hipSuccess) {
            (void) hipGetLastError();
            return fail(BF_ERR_NOMEM, "%s shape %u: hipMalloc(%zu bytes) for the normal index: %s", who, shape,
                        off.size() * sizeof(uint32_t) + n_corners * sizeof(uint4), hipGetErrorString(he));
        }
        HIP_TRY(hipMemcpy(idx->offset, off.data(), off.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (n_corners) HIP_TRY(hipMemcpy(idx->entries, ent.data(), n_corners * sizeof(uint4), hipMemcpyHostToDevice));
        g.normal_index[shape] = std::move(idx);
    }
    *out = g.normal_index[shape].get();
    return BF_OK;
}

// while a chunk renders, the handle's kernel arguments point at version 0 of the arena; restored on every return path
struct GeomSwap {
    bf_scene *s;
    bfd::DScene saved;
    GeomSwap(bf_scene *sc, const bfd::DScene &view) : s(sc), saved(sc->d) { sc->d = view; }
    ~GeomSwap() { s->d = saved; }
};

// default arena budget of the batches (BF_MOTION_BATCH_MB overrides it at call time)
constexpr size_t kMotionBatchMB = 2048;

// What motion and deform batches share: chunks of renders whose versions fit the arena budget (BF_MOTION_BATCH_MB; at least one render
// per chunk), the arena grown on demand, and per chunk prepare(k0, kc, a, L), which enqueues the chunk's versions into the arena `a`,
// then the chunk's renders with the handle's kernel arguments pointing at version 0.  `fn` names the caller in error text.
template <class Prepare>
bf_status render_versions(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, float *hist_dev,
                          bf_path_record *records_dev, void *stream_, bf_stats *stats_out, const char *fn, Prepare &&prepare) {
    MeshState &m = scene->mesh;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const uint64_t n_chan = bf_scene_launch_channels(scene, launch);      // floats per render (x n_classes under BF_FLAG_CLASSES; the AOV layout under BF_FLAG_AOV)
    // Velocity modes (bf_velocity.h): a shape in BF_VELOCITY_DIFFERENCE takes its field from consecutive versions, so a chunk is
    // prepared with the first version of the next chunk behind it; the rows are built (and count towards the budget) only for a
    // launch that can read them, a class launch under a range-rate table.
    const bool with_vel = m.velocities() && (launch->flags & BF_FLAG_CLASSES) && bfd::scene_class_range_rate(scene->d) && m.vel && m.vel_tab;
    const bool diff = with_vel && m.differences();
    if (diff && n_renders < 2)
        return fail(BF_ERR_INVALID, "%s: n_renders is 1: a shape of this scene is in BF_VELOCITY_DIFFERENCE, whose velocities are the differences "
                                    "of consecutive renders (at least 2)", fn);
    const MotionLayout L = motion_layout(scene->d, with_vel);
    if (L.rows > UINT32_MAX)
        return fail(BF_ERR_UNSUPPORTED, "%s: one geometry version of this scene is %zu float4 rows (at most 2^32 - 1)", fn, L.rows);
    size_t budget_mb = kMotionBatchMB;
    if (const char *e = getenv("BF_MOTION_BATCH_MB")) {
        char *end = nullptr;
        const unsigned long long v = strtoull(e, &end, 10);
        if (end != e && *end == '\0') budget_mb = (size_t) v;
    }
    const size_t version_bytes = L.rows * sizeof(float4);
    const uint32_t per_chunk = (uint32_t) std::max<size_t>(1, std::min<size_t>({(size_t) n_renders, (size_t) (diff ? 65534 : 65535),(budget_mb << 20) / version_bytes}));
    const size_t need = ((size_t) per_chunk + (diff ? 1 : 0)) * L.rows;      // (diff: the next chunk's first version)
    if (m.arena_cap < need) {
        // the old arena may still be read by the renders of an earlier call: wait for them before it goes
        if (m.arena) {
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(hipFree(m.arena));
            m.arena = nullptr;
            m.arena_cap = 0;
        }
        void *q = nullptr;
        hipError_t he = hipMalloc(&q, need * sizeof(float4));
        if (he != hipSuccess)
            return fail(BF_ERR_NOMEM, "%s: hipMalloc(%zu bytes) for %u geometry versions: %s (BF_MOTION_BATCH_MB caps the arena)", fn,
                        need * sizeof(float4), per_chunk, hipGetErrorString(he));
        m.arena = (float4 *) q;
        m.arena_cap = need;
    }
    float4 *const a = m.arena;
    bfd::DScene view = scene->d;
    view.tris = a + L.tris;
    view.normals = scene->d.normals ? a + L.normals : nullptr;
    view.nodes = a + L.nodes;
    view.wnodes = scene->d.wnodes ? a + L.wnodes : nullptr;
    view.qnodes = scene->d.qnodes ? a + L.qnodes : nullptr;
    if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
    m.batch_versions = 0;
    m.batch_vel = with_vel;
    // while the chunks render, the range-rate table names the arena's velocity rows; the handle's own again on every return path
    struct VelStamp {
        bf_scene *s;
        hipStream_t stream;
        bool on;
        ~VelStamp() {
            if (on) (void) velocity_stamp(s, s->mesh.vel, stream);
        }
    } vel_stamp{scene, stream, false};
    if (with_vel) {
        const bf_status vst = velocity_stamp(scene, a + L.vel, stream);
        if (vst != BF_OK) return vst;
        vel_stamp.on = true;
    }
    for (uint32_t k0 = 0; k0 < n_renders; k0 += per_chunk) {
        const uint32_t kc = std::min(per_chunk, n_renders - k0);
        const bool final = k0 + kc == n_renders;
        bf_status st = prepare(k0, diff && !final ? kc + 1u : kc, a, L);
        if (st != BF_OK) return st;
        if (with_vel) {
            // the last version of the chunk: against the next chunk's first; the batch's last render: the field of the one before it
            uint32_t tail_prev = kc - 1u, tail_next = diff && !final ? kc : kc - 1u;
            if (diff && final && kc >= 2u) tail_prev = kc - 2u;
            // (a last chunk of one render prepares version n - 2 once more, whole, pose, gather and refit, for its triangle rows alone,
            // and a batch cut to one render per chunk prepares every version twice: redundant work where the budget is that tight,
            // accepted for one way of making a version)
            if (diff && final && kc == 1u) {
                if ((st = prepare(n_renders - 2u, 1u, a + L.rows, L)) != BF_OK) return st;
                tail_prev = 1u, tail_next = 0u;
            }
            HIP_TRY(bfk_launch_velocity_diff(a + L.tris, a + L.tris, a + L.vel, m.vel, scene->d.n_tris, m.vel_tab, kc, L.rows, tail_prev, tail_next,
                                             stream));
        }
        bf_batch b = {kc, seeds ? seeds + k0 : nullptr, nullptr};
        bf_stats cs;
        {
            GeomSwap swap(scene, view);
            st = render_locked(scene, launch, &b, hist_dev + (size_t) k0 * n_chan, records_dev ? records_dev + (size_t) k0 * launch->n_paths : nullptr,
                               stream_, stats_out ? &cs : nullptr, (uint32_t) L.rows);
        }
        if (st != BF_OK) return st;
        if (stats_out) add_stats(*stats_out, cs);
    }
    if (n_renders <= per_chunk) m.batch_versions = n_renders, m.batch_rows = L.rows;
    return BF_OK;
}

}  // namespace

bf_status MeshState::own_normals(bfd::DScene &d, std::vector<void *> &owned, const char *who) {
    if (!d.normals || normals_private) return BF_OK;
    float4 *q = nullptr;
    const bf_status st = DevAlloc{owned, who}(bytes(d).normals, &q);
    if (st != BF_OK) return st;
    if (!normals0) normals0 = const_cast<float4 *>(d.normals);
    d.normals = q;
    normals_private = true;
    return BF_OK;
}

void MeshState::reset_after_rebuild(float4 *tris0_, float4 *nodes0_, float4 *wnodes0_, float4 *normals0_) {
    const bool posed = tris0_ != nullptr;
    tris0 = tris0_, nodes0 = nodes0_, wnodes0 = wnodes0_, normals0 = normals0_;
    // the handle's own arrays throughout; the boxes kept beside a pose are the POSED geometry's: only their topology is read from now on
    geom_private = base_private = posed;
    normals_private = normals0_private = normals0_ != nullptr;
    if (posed) deformed = true;
    // the level lists follow the topology: rebuilt at the next refit (mesh boxes and transform table stay); the arena's layout has changed
    refit.ready = false;
    refit.lvl4 = refit.lvl16 = nullptr;
    refit.ubox4 = refit.ubox16 = nullptr;
    refit.off4.clear();
    refit.off16.clear();
    batch_versions = 0;
}

MeshState::~MeshState() {
    if (arena) (void) hipFree(arena);
    if (bad) (void) hipFree(bad);
    if (bad_host) (void) hipHostFree(bad_host);
    if (bad_ev) (void) hipEventDestroy(bad_ev);
    if (vtx_ev) {
        (void) hipEventSynchronize(vtx_ev);
        (void) hipEventDestroy(vtx_ev);
    }
    if (vtx_host) (void) hipHostFree(vtx_host);
    if (vtx_dev) (void) hipFree(vtx_dev);
    if (pose_vtx) (void) hipFree(pose_vtx);
    if (nrm_vtx) (void) hipFree(nrm_vtx);
    if (vel) (void) hipFree(vel);
    if (vel_prev) (void) hipFree(vel_prev);
    if (vel_tab) (void) hipFree(vel_tab);
}

extern "C" {

bf_status deform_report(const bf_scene *scene, bool wait) {
    const MeshState &m = scene->mesh;
    if (!m.bad_pending) return BF_OK;
    if (wait) {
        HIP_TRY(hipEventSynchronize(m.bad_ev));
    } else if (hipEventQuery(m.bad_ev) != hipSuccess) {
        (void) hipGetLastError();
        return BF_OK;
    }
    m.bad_pending = false;
    // the device counter only ever grows (nothing clears it under a gather in flight): what is new since the last report
    const uint32_t total = m.bad_host[0], shape1 = m.bad_host[1];
    const uint32_t n = total - m.bad_reported;
    m.bad_reported = total;
    if (!n) return BF_OK;
    return fail(BF_ERR_DEVICE, "a device-form vertex update of this scene gave %u triangles (of shape %u, if not of others too) a corner "
                               "that is not finite or lies beyond the declared bound: those triangles kept their previous vertices, "
                               "and every render issued since that update is invalid", n, shape1 ? shape1 - 1u : 0u);
}

bf_status check_deform_shape(const bf_scene *scene, uint32_t shape, bool with_normals, const char *who, const bf_geometry::MeshTopo **topo_out) {
    if (shape >= scene->info.n_shapes) return fail(BF_ERR_INVALID, "%s shape %u: the scene has %u shapes", who, shape, scene->info.n_shapes);
    const bfd::DShape &sh = scene->ends.shapes_host[shape];
    if (sh.type != BF_SHAPE_MESH) return fail(BF_ERR_INVALID, "%s shape %u is not a mesh", who, shape);
    if (sh.emitter >= 0)
        return fail(BF_ERR_UNSUPPORTED, "%s mesh shape %u carries emitter %d (its sampling tables are built from the triangles as "
                                        "created); create a new scene", who, shape, sh.emitter);
    const bf_geometry::MeshTopo &tp = scene->geom->topo[shape];
    if (with_normals && !tp.has_normals)
        return fail(BF_ERR_INVALID, "%s shape %u was created without vertex normals: it cannot take any", who, shape);
    *topo_out = &tp;
    return BF_OK;
}

bf_status mesh_clone_snapshot(const bf_scene *src, bf_scene *sc) {
    const MeshState &m = src->mesh;
    sc->mesh.origin_scale_built = m.origin_scale_built;
    sc->mesh.skins = m.skins;      // shared, never written: bf_scene_set_skin on either handle replaces that handle's pointer alone
    sc->mesh.morphs = m.morphs;    // likewise (bf_scene_set_morph)
    sc->mesh.normal_mode = m.normal_mode;      // the source's modes at this moment; the clone's own from now on
    sc->mesh.skin_mode = m.skin_mode;          // likewise (bf_scene_set_skin_mode)
    // ... and the velocity modes, time steps and field (bf_scene_set_velocity_mode): the clone's own rows, in the slot order both share now
    sc->mesh.vel_mode = m.vel_mode;
    sc->mesh.vel_dt = m.vel_dt;
    if (m.vel && m.vel_tab) {
        const size_t vel_bytes = (size_t) src->d.n_tris * bfvel::kRowsPerSlot * sizeof(float4), tab_bytes = (size_t) src->info.n_shapes * sizeof(float2);
        hipError_t he = hipMalloc((void **) &sc->mesh.vel, vel_bytes);
        if (he == hipSuccess) he = hipMalloc((void **) &sc->mesh.vel_tab, tab_bytes);
        if (he != hipSuccess) {
            (void) hipGetLastError();
            return fail(BF_ERR_NOMEM, "bf_scene_clone: hipMalloc(%zu bytes) for the velocity rows: %s", vel_bytes + tab_bytes, hipGetErrorString(he));
        }
        HIP_TRY(hipMemcpy(sc->mesh.vel, m.vel, vel_bytes, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(sc->mesh.vel_tab, m.vel_tab, tab_bytes, hipMemcpyDeviceToDevice));
    }
    if (!m.tris0 && !m.geom_private) return BF_OK;
    // `src` has moved: the clone snapshots what src renders now as ITS geometry "as created"; uvs (and normals no transform moved) stay shared
    const MeshState::Bytes B = MeshState::bytes(src->d);
    DevAlloc take{sc->owned, "bf_scene_clone"};
    auto dup = [&](const float4 *from, size_t bytes, const float4 **to) -> bf_status {
        float4 *p = nullptr;
        const bf_status st = take(from ? bytes : 0, &p);
        if (p) HIP_TRY(hipMemcpy(p, from, bytes, hipMemcpyDeviceToDevice));
        *to = p;
        return st;
    };
    bf_status st = BF_OK;
    if ((st = dup(src->d.tris, B.tris, &sc->d.tris)) != BF_OK) return st;
    if ((st = dup(src->d.nodes, B.nodes, &sc->d.nodes)) != BF_OK) return st;
    if ((st = dup(src->d.wnodes, B.wnodes, &sc->d.wnodes)) != BF_OK) return st;
    if (src->d.qnodes && (st = dup(src->d.qnodes, B.nodes / 2, &sc->d.qnodes)) != BF_OK) return st;
    // normals a rigid transform moved are part of the snapshot (never written: the clone's first transform moves them into another array)
    if (m.normals_private && (st = dup(src->d.normals, B.normals, &sc->d.normals)) != BF_OK) return st;
    sc->mesh.geom_private = true;
    sc->geom_token = std::make_shared<char>(0);      // the snapshot is the clone's alone: `src` keeps translating in place
    return BF_OK;
}

// ---- velocity rows (bf_scene_set_velocity_mode) -----------------------------------------------------------------------
bf_status velocity_before(bf_scene *scene, hipStream_t stream) {
    MeshState &m = scene->mesh;
    if (!m.differences() || !m.vel) return BF_OK;
    const size_t bytes = (size_t) scene->d.n_tris * bfd::kTriStride * sizeof(float4);
    if (!m.vel_prev) {
        const hipError_t he = hipMalloc((void **) &m.vel_prev, bytes);
        if (he != hipSuccess) {
            (void) hipGetLastError();
            return fail(BF_ERR_NOMEM, "hipMalloc(%zu bytes) for the triangle rows a velocity difference starts from: %s", bytes, hipGetErrorString(he));
        }
    }
    HIP_TRY(hipMemcpyAsync(m.vel_prev, scene->d.tris, bytes, hipMemcpyDeviceToDevice, stream));
    return BF_OK;
}
bf_status velocity_after(bf_scene *scene, uint32_t shape, hipStream_t stream) {
    MeshState &m = scene->mesh;
    if (!m.differences() || !m.vel || !m.vel_prev) return BF_OK;
    if (shape != kAllShapes && m.velocity_mode(shape) != BF_VELOCITY_DIFFERENCE) return BF_OK;
    // One version, its output the handle's own rows: the kernel leaves the slots of every shape it is not told to difference as they
    // are.  A call that moved one shape tells it that shape alone (a table of the call's own: every other shape reads as
    // BF_VELOCITY_TWIST), so a shape the call did not move keeps its field, though the pose has rewritten its rows with what they held.
    const float2 *tab = m.vel_tab;
    if (shape != kAllShapes) {
        const size_t bytes = (size_t) scene->info.n_shapes * sizeof(float2);
        bf_scene::Stage *stg = nullptr;
        bf_status st = stage_acquire(scene, bytes, &stg);
        if (st != BF_OK) return st;
        std::memset(stg->host, 0, bytes);
        const uint32_t bits = BF_VELOCITY_DIFFERENCE;
        float2 &e = ((float2 *) stg->host)[shape];
        std::memcpy(&e.x, &bits, 4);
        e.y = m.vel_dt[shape];
        if ((st = stage_commit(stg, bytes, stream)) != BF_OK) return st;
        tab = (const float2 *) stg->dev;
        HIP_TRY(bfk_launch_velocity_diff(m.vel_prev, scene->d.tris, m.vel, m.vel, scene->d.n_tris, tab, 1u, 0u, 0u, 0u, stream));
        HIP_TRY(hipEventRecord(stg->ev, stream));      // the table is read by the kernel, not only by the copy
        return BF_OK;
    }
    HIP_TRY(bfk_launch_velocity_diff(m.vel_prev, scene->d.tris, m.vel, m.vel, scene->d.n_tris, tab, 1u, 0u, 0u, 0u, stream));
    return BF_OK;
}

// ---- what bf_pose.cpp calls too (bf_scene.h) ----------------------------------------------------------------------------------------
// the prologue of every call that moves meshes: behind the handle's previous work, with its open rolling sequence ended
bf_status mesh_enter(const bf_scene *scene, hipStream_t stream) {
    const bf_status st = order_after_last(scene, stream);
    return st == BF_OK ? close_sequence(scene, stream) : st;
}

// check_rigid_table of every render of a batch (to_world: [n_renders][n_shapes][12]); `fn` ends in ':'
bf_status check_rigid_tables(const bf_scene *scene, const char *fn, uint32_t n_renders, uint32_t n_shapes, const float *to_world, uint8_t *moves) {
    for (uint32_t k = 0; k < n_renders; ++k) {
        char who[96];
        std::snprintf(who, sizeof(who), "%s render %u,", fn, k);
        const bf_status st = check_rigid_table(scene, n_shapes, to_world + (size_t) 12 * n_shapes * k, who, moves + (size_t) n_shapes * k);
        if (st != BF_OK) return st;
    }
    return BF_OK;
}

// A scratch buffer of the handle's own (posed vertices, recomputed normals), at least `bytes`: grown on demand, never shrunk (the
// gathers that read the old one are behind `stream` or before it: mesh_enter).  `what` names its content in the error text.
bf_status vertex_scratch(float *&buf, size_t &cap, size_t bytes, hipStream_t stream, const char *who, const char *what) {
    if (cap >= bytes) return BF_OK;
    if (buf) {
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipFree(buf));
        buf = nullptr;
        cap = 0;
    }
    void *q = nullptr;
    const hipError_t he = hipMalloc(&q, bytes);
    if (he != hipSuccess) {
        (void) hipGetLastError();
        return fail(BF_ERR_NOMEM, "%s hipMalloc(%zu bytes) for the %s: %s", who, bytes, what, hipGetErrorString(he));
    }
    buf = (float *) q;
    cap = bytes;
    return BF_OK;
}

// one update with the arrays on the device already; box6: the new base box of the shape
bf_status update_vertices_locked(bf_scene *scene, uint32_t shape, const bf_geometry::MeshTopo &tp, const float *pos_dev, const float *nrm_dev,
                                 float bound, const float *box6, bool watch, hipStream_t stream) {
    const char *who = "bf_scene_update_vertices";
    MeshState &m = scene->mesh;
    bf_status st = BF_OK;
    if (!m.refit.ready && (st = refit_prepare(scene, stream)) != BF_OK) return st;
    if ((st = deform_prepare(scene, stream)) != BF_OK) return st;
    // BF_NORMALS_RECOMPUTE and no normals in the call: the statement of the new positions into the handle's scratch, gathered below
    // as if the caller had given them (and watched like a device form: finite positions may have cross products that are not)
    const bool recompute = !nrm_dev && scene->d.normals && m.recomputes(shape);
    const bf_geometry::NormalIndex *nidx = nullptr;
    if (recompute) {
        if ((st = normal_index(scene, shape, who, &nidx)) != BF_OK) return st;
        if ((st = vertex_scratch(m.nrm_vtx, m.nrm_vtx_cap, (size_t) tp.n_vertices * 3 * sizeof(float), stream, who, "recomputed normals")) != BF_OK) return st;
    }
    if ((st = own_geometry(scene, stream, who)) != BF_OK) return st;
    if (recompute) {
        HIP_TRY(bfk_launch_vertex_normals(nidx->offset, nidx->entries, tp.n_vertices, pos_dev, m.nrm_vtx, 1u, stream));
        nrm_dev = m.nrm_vtx;
        watch = true;
    }
    const MeshState::Bytes B = MeshState::bytes(scene->d);
    DevAlloc take{scene->owned, who};
    if (!m.base_private) {
        // the base rows are still the arrays shared with clones: this handle's own copy from now on
        float4 *q = nullptr;
        if ((st = take(B.tris, &q)) != BF_OK) return st;
        HIP_TRY(hipMemcpyAsync(q, m.tris0, B.tris, hipMemcpyDeviceToDevice, stream));
        m.tris0 = q;
        m.base_private = true;
    }
    if ((st = m.own_normals(scene->d, scene->owned, who)) != BF_OK) return st;
    if (nrm_dev && !m.normals0_private) {
        float4 *q = nullptr;
        if ((st = take(B.normals, &q)) != BF_OK) return st;
        HIP_TRY(hipMemcpyAsync(q, m.normals0, B.normals, hipMemcpyDeviceToDevice, stream));
        m.normals0 = q;
        m.normals0_private = true;
    }
    // the per-shape source table: this shape alone deforms
    const size_t bytes = (size_t) scene->info.n_shapes * sizeof(bfd::DDeformSrc);
    bf_scene::Stage *stg = nullptr;
    if ((st = stage_acquire(scene, bytes, &stg)) != BF_OK) return st;
    std::memset(stg->host, 0, bytes);
    bfd::DDeformSrc &e = ((bfd::DDeformSrc *) stg->host)[shape];
    e.pos = pos_dev;
    e.nrm = nrm_dev;
    e.nv = tp.n_vertices;
    if ((st = stage_commit(stg, bytes, stream)) != BF_OK) return st;
    HIP_TRY(bfk_launch_deform_tris(scene->geom->corners, (const bfd::DDeformSrc *) stg->dev, m.tris0, m.tris0, nrm_dev ? m.normals0 : nullptr,
                                   nrm_dev ? m.normals0 : nullptr, scene->d.n_tris, nullptr, 1u, 0u, 0u, bound, m.bad, stream));
    HIP_TRY(hipEventRecord(stg->ev, stream));      // the table is read by the kernel, not only by the copy
    if (watch && (st = deform_watch(scene, stream)) != BF_OK) return st;
    std::memcpy(&m.refit.mesh_box[6 * (size_t) shape], box6, 6 * sizeof(float));
    m.deformed = true;
    return apply_pose(scene, stream);
}

// What deform and posed batches share behind their checks: version k = the shapes of `src` (pos != nullptr; one entry per shape of the
// scene) gathered from their arrays, every other mesh from the handle's base rows, then to_world[k] (absolute; NULL: none; `moves` from
// check_rigid_tables), both trees re-fitted.  slice(k0, kc, hs) turns the copy `hs` of `src` into the table of renders k0 .. k0 + kc (it
// may enqueue what fills the arrays first); `bound` covers every array of the call.  `who` names the caller in error text.
bf_status deform_versions(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, const std::vector<bfd::DDeformSrc> &src,
                          float bound, const float *to_world, const std::vector<uint8_t> &moves, float *hist_dev, bf_path_record *records_dev,
                          void *stream_, bf_stats *stats_out, const char *who, const DeformSlice &slice) {
    MeshState &m = scene->mesh;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const uint32_t n_shapes = scene->info.n_shapes;
    bool any = false;
    for (const bfd::DDeformSrc &e : src) any = any || e.pos != nullptr;
    bf_status st = BF_OK;
    if ((st = mesh_enter(scene, stream)) != BF_OK) return st;
    if (!m.refit.ready && (st = refit_prepare(scene, stream)) != BF_OK) return st;
    if ((st = deform_prepare(scene, stream)) != BF_OK) return st;
    // BF_NORMALS_RECOMPUTE: a listed shape without normals of its own in this call gets them from each version's (untransformed)
    // positions, behind `slice` below; its index is built here, before anything is enqueued
    std::vector<const bf_geometry::NormalIndex *> nidx(n_shapes, nullptr);
    size_t nrm_floats = 0;      // per render, over the recomputing shapes
    for (uint32_t k = 0; k < n_shapes; ++k) {
        if (!src[k].pos || src[k].nrm || !scene->d.normals || !m.recomputes(k)) continue;
        if ((st = normal_index(scene, k, who, &nidx[k])) != BF_OK) return st;
        nrm_floats += (size_t) src[k].nv * 3;
    }
    // one padding bound for all versions: the handle's, raised over every mesh of every render (a deforming shape's box: [-bound, bound]^3)
    float oscale = m.origin_scale_built;
    {
        std::vector<float> box = m.refit.mesh_box, id((size_t) 12 * n_shapes);
        for (uint32_t k = 0; k < n_shapes; ++k) {
            id[12 * (size_t) k] = id[12 * (size_t) k + 5] = id[12 * (size_t) k + 10] = 1.f;
            if (src[k].pos)
                for (int a = 0; a < 3; ++a) box[6 * (size_t) k + a] = -bound, box[6 * (size_t) k + 3 + a] = bound;
        }
        oscale = origin_bound(box, n_shapes, id.data(), 12, nullptr, oscale);
        for (uint32_t k = 0; to_world && k < n_renders; ++k)
            oscale = origin_bound(box, n_shapes, to_world + (size_t) 12 * n_shapes * k, 12, moves.data() + (size_t) n_shapes * k, oscale);
    }
    st = render_versions(scene, launch, n_renders, seeds, hist_dev, records_dev, stream_, stats_out, who,
                         [&](uint32_t k0, uint32_t kc, float4 *a, const MotionLayout &L) -> bf_status {
        // the chunk's tables: the sources as `slice` leaves them for renders k0 .. k0 + kc, then (if any) the transforms
        const size_t src_bytes = (src.size() * sizeof(bfd::DDeformSrc) + 15) & ~size_t(15), n = to_world ? (size_t) kc * n_shapes : 0;
        const size_t bytes = src_bytes + n * 16 * sizeof(float);
        bf_scene::Stage *stg = nullptr;
        bf_status pst = stage_acquire(scene, bytes, &stg);
        if (pst != BF_OK) return pst;
        bfd::DDeformSrc *hs = (bfd::DDeformSrc *) stg->host;
        for (uint32_t k = 0; k < n_shapes; ++k) hs[k] = src[k];
        if ((pst = slice(k0, kc, hs)) != BF_OK) return pst;
        if (nrm_floats) {
            // the chunk's recomputed normals: per shape [kc][nv][3], one shape after the other, version v of the gather reads slice v
            if ((pst = vertex_scratch(m.nrm_vtx, m.nrm_vtx_cap, (size_t) kc * nrm_floats * sizeof(float), stream, who, "recomputed normals")) != BF_OK)
                return pst;
            float *out = m.nrm_vtx;
            for (uint32_t k = 0; k < n_shapes; ++k) {
                if (!nidx[k]) continue;
                HIP_TRY(bfk_launch_vertex_normals(nidx[k]->offset, nidx[k]->entries, hs[k].nv, hs[k].pos, out, kc, stream));
                hs[k].nrm = out;
                out += (size_t) kc * hs[k].nv * 3;
            }
        }
        if (n) pack_rigid((float *) ((char *) stg->host + src_bytes), to_world + 12 * (size_t) k0 * n_shapes, moves.data() + (size_t) k0 * n_shapes, n);
        if ((pst = stage_commit(stg, bytes, stream)) != BF_OK) return pst;
        const MeshState::Base b = m.base(scene->d);
        const RefitDst o = arena_dst(scene, a, L, kc);
        HIP_TRY(bfk_launch_deform_tris(scene->geom->corners, (const bfd::DDeformSrc *) stg->dev, b.tris, o.tris, b.normals, o.normals, scene->d.n_tris,
                                       to_world ? (const float *) ((const char *) stg->dev + src_bytes) : nullptr, kc, L.rows, n_shapes * 16u, bound,
                                       m.bad, stream));
        HIP_TRY(hipEventRecord(stg->ev, stream));      // the tables are read by the kernel
        HIP_TRY(launch_refit(scene, oscale, o, stream));
        return BF_OK;
    });
    if (st != BF_OK || !any) return st;
    // the violation count of all chunks travels to the host behind the last one; a batch with stats waits for it and reports itself
    if ((st = deform_watch(scene, stream)) != BF_OK) return st;
    return stats_out ? deform_report(scene, true) : BF_OK;
}

// The refusals every batch with a geometry version per render has before it looks at its tables: `fn` ends in ':', `kind` is "motion",
// "deform", "skin" or "morph"; to_world may be NULL (then n_shapes is not looked at).
bf_status check_batch_call(const char *fn, const char *kind, const bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const float *to_world,
                           uint32_t n_shapes, const float *hist_dev) {
    if (!scene || !launch || !hist_dev) return fail(BF_ERR_INVALID, "%s null argument", fn);
    if (n_renders == 0) return fail(BF_ERR_INVALID, "%s n_renders is 0", fn);
    if (to_world && n_shapes != scene->info.n_shapes)
        return fail(BF_ERR_INVALID, "%s %u transforms per render for a scene of %u shapes", fn, n_shapes, scene->info.n_shapes);
    if (launch->flags & BF_FLAG_ROLLING) return fail(BF_ERR_INVALID, "%s BF_FLAG_ROLLING: a %s batch is one launch sequence of its own", fn, kind);
    if (launch->spp && launch->film_width && launch->film_height)
        return fail(BF_ERR_INVALID, "%s multi-pixel films are rendered one launch at a time", fn);
    return BF_OK;
}

// ... and what each does first behind the lock.  A refused class, AOV or exact-sum launch does no device work (the refit's preparation and the
// geometry versions would come first), and a scene without triangles has nothing to move: an ordinary batch.  True: the call ends
// here with *st; false: the caller goes on to its versions.
bool batch_ends_early(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, float *hist_dev,
                      bf_path_record *records_dev, void *stream_, bf_stats *stats_out, bf_status *st) {
    if ((*st = check_classes(scene, launch, n_renders)) != BF_OK || (*st = check_aov(scene, launch, n_renders)) != BF_OK ||
        (*st = check_sum(scene, launch, n_renders)) != BF_OK)
        return true;
    if (scene->d.n_tris != 0) return false;
    bf_batch b = {n_renders, seeds, nullptr};
    *st = render_locked(scene, launch, &b, hist_dev, records_dev, stream_, stats_out);
    return true;
}

bf_status bf_scene_translate_meshes(bf_scene *scene, const float offset[3], void *stream_) {
    if (!scene || !offset) return fail(BF_ERR_INVALID, "null argument");
    if (!(std::isfinite(offset[0]) && std::isfinite(offset[1]) && std::isfinite(offset[2])))
        return fail(BF_ERR_INVALID, "bf_scene_translate_meshes: non-finite offset");
    if (scene->d.n_tris == 0) return BF_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    const bfd::DScene &d = scene->d;
    bf_status st = mesh_enter(scene, stream);
    if (st != BF_OK) return st;
    if ((st = velocity_before(scene, stream)) != BF_OK) return st;
    if (m.deformed && !m.refit.ready && (st = refit_prepare(scene, stream)) != BF_OK) return st;
    if ((st = own_geometry(scene, stream, __func__)) != BF_OK) return st;
    m.pose_kind = 1;      // [I | offset] for every shape
    m.pose_xf.assign((size_t) scene->info.n_shapes * 16, 0.f);
    for (uint32_t k = 0; k < scene->info.n_shapes; ++k) {
        float *x = &m.pose_xf[16 * (size_t) k];
        x[0] = x[5] = x[10] = x[12] = 1.f;
        x[3] = offset[0], x[7] = offset[1], x[11] = offset[2];
    }
    if (m.deformed) {
        // nodes0 / wnodes0 do not bound the base rows: the same vertices (fl(v + offset) either way) under re-fitted boxes
        if ((st = apply_pose(scene, stream)) != BF_OK || (st = velocity_after(scene, kAllShapes, stream)) != BF_OK) return st;
        return mark_last(scene, stream);
    }
    if (m.normals_moved) {
        // a rigid transform moved the vertex normals: a translation applies to the geometry as created
        HIP_TRY(hipMemcpyAsync(const_cast<float4 *>(d.normals), m.normals0, MeshState::bytes(d).normals, hipMemcpyDeviceToDevice, stream));
        m.normals_moved = false;
    }
    HIP_TRY(bfk_launch_translate(m.tris0, const_cast<float4 *>(d.tris), d.n_tris * bfd::kTriStride, m.nodes0, const_cast<float4 *>(d.nodes),
                                 const_cast<float4 *>(d.qnodes), d.n_nodes, m.wnodes0, const_cast<float4 *>(d.wnodes),
                                 d.wnodes ? d.n_wnodes * 16u : 0u, offset, stream));
    if ((st = velocity_after(scene, kAllShapes, stream)) != BF_OK) return st;
    return mark_last(scene, stream);
}

bf_status bf_scene_transform_meshes(bf_scene *scene, uint32_t n_shapes, const float *to_world, void *stream_) {
    if (!scene || !to_world) return fail(BF_ERR_INVALID, "null argument");
    if (n_shapes != scene->info.n_shapes)
        return fail(BF_ERR_INVALID, "bf_scene_transform_meshes: %u transforms for a scene of %u shapes", n_shapes, scene->info.n_shapes);
    // everything is checked before anything changes: a failed call leaves the scene as it was
    std::vector<uint8_t> moves(n_shapes, 0);
    bf_status st = check_rigid_table(scene, n_shapes, to_world, "bf_scene_transform_meshes:", moves.data());
    if (st != BF_OK) return st;
    if (scene->d.n_tris == 0) return BF_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    if ((st = mesh_enter(scene, stream)) != BF_OK) return st;
    if ((st = velocity_before(scene, stream)) != BF_OK) return st;
    if (!m.refit.ready && (st = refit_prepare(scene, stream)) != BF_OK) return st;
    if ((st = own_geometry(scene, stream, __func__)) != BF_OK) return st;
    if ((st = m.own_normals(scene->d, scene->owned, __func__)) != BF_OK) return st;      // the vertex normals move too
    // ray origins now lie on the moved meshes: raise (never lower) the padding bound over the MOVED ones (apply_pose's adds a margin on all)
    m.origin_scale_built = origin_bound(m.refit.mesh_box, n_shapes, to_world, 12, moves.data(), m.origin_scale_built);
    m.pose_kind = 2;
    m.pose_xf.resize((size_t) n_shapes * 16);
    pack_rigid(m.pose_xf.data(), to_world, moves.data(), n_shapes);
    if ((st = run_pose(scene, stream)) != BF_OK || (st = velocity_after(scene, kAllShapes, stream)) != BF_OK) return st;
    return mark_last(scene, stream);
}

bf_status bf_scene_update_vertices(bf_scene *scene, uint32_t shape, const float *positions, const float *normals, void *stream_) {
    if (!scene || !positions) return fail(BF_ERR_INVALID, "bf_scene_update_vertices: null argument");
    const bf_geometry::MeshTopo *tp = nullptr;
    bf_status st = check_deform_shape(scene, shape, normals != nullptr, "bf_scene_update_vertices:", &tp);
    if (st != BF_OK) return st;
    const size_t n = 3 * (size_t) tp->n_vertices;
    const float inf = std::numeric_limits<float>::infinity();
    float box[6] = {inf, inf, inf, -inf, -inf, -inf};
    for (size_t i = 0; i < n; ++i) {
        if (!std::isfinite(positions[i]) || (normals && !std::isfinite(normals[i])))
            return fail(BF_ERR_INVALID, "bf_scene_update_vertices: shape %u: non-finite value at vertex %zu", shape, i / 3);
        box[i % 3] = std::min(box[i % 3], positions[i]);
        box[3 + i % 3] = std::max(box[3 + i % 3], positions[i]);
    }
    if (scene->d.n_tris == 0 || n == 0) return BF_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    if ((st = mesh_enter(scene, stream)) != BF_OK) return st;
    if ((st = velocity_before(scene, stream)) != BF_OK) return st;
    // the caller's arrays through the handle's upload buffer (the staging ring is for small tables): free again on return
    const size_t bytes = n * sizeof(float) * (normals ? 2 : 1);
    if (m.vtx_ev) HIP_TRY(hipEventSynchronize(m.vtx_ev));      // the previous update's gather may still read it
    if (m.vtx_cap < bytes) {
        if (m.vtx_host) (void) hipHostFree(m.vtx_host);
        if (m.vtx_dev) (void) hipFree(m.vtx_dev);
        m.vtx_host = m.vtx_dev = nullptr;
        m.vtx_cap = 0;
        HIP_TRY(hipHostMalloc(&m.vtx_host, bytes));
        HIP_TRY(hipMalloc(&m.vtx_dev, bytes));
        m.vtx_cap = bytes;
    }
    if (!m.vtx_ev) HIP_TRY(hipEventCreateWithFlags(&m.vtx_ev, hipEventDisableTiming));
    std::memcpy(m.vtx_host, positions, n * sizeof(float));
    if (normals) std::memcpy((float *) m.vtx_host + n, normals, n * sizeof(float));
    HIP_TRY(hipMemcpyAsync(m.vtx_dev, m.vtx_host, bytes, hipMemcpyHostToDevice, stream));
    st = update_vertices_locked(scene, shape, *tp, (const float *) m.vtx_dev, normals ? (const float *) m.vtx_dev + n : nullptr, inf, box, false, stream);
    HIP_TRY(hipEventRecord(m.vtx_ev, stream));
    if (st != BF_OK || (st = velocity_after(scene, shape, stream)) != BF_OK) return st;
    return mark_last(scene, stream);
}

bf_status bf_scene_update_vertices_device(bf_scene *scene, uint32_t shape, const float *positions_dev, const float *normals_dev, float bound,
                                          void *stream_) {
    if (!scene || !positions_dev) return fail(BF_ERR_INVALID, "bf_scene_update_vertices_device: null argument");
    if (!(bound > 0.f) || !std::isfinite(bound)) return fail(BF_ERR_INVALID, "bf_scene_update_vertices_device: shape %u: bound must be positive and finite", shape);
    const bf_geometry::MeshTopo *tp = nullptr;
    bf_status st = check_deform_shape(scene, shape, normals_dev != nullptr, "bf_scene_update_vertices_device:", &tp);
    if (st != BF_OK) return st;
    if (scene->d.n_tris == 0 || tp->n_vertices == 0) return BF_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    if ((st = mesh_enter(scene, stream)) != BF_OK) return st;
    if ((st = velocity_before(scene, stream)) != BF_OK) return st;
    const float box[6] = {-bound, -bound, -bound, bound, bound, bound};
    if ((st = update_vertices_locked(scene, shape, *tp, positions_dev, normals_dev, bound, box, true, stream)) != BF_OK) return st;
    if ((st = velocity_after(scene, shape, stream)) != BF_OK) return st;
    return mark_last(scene, stream);
}

// ---- recomputed normals: the host statement and the per-shape mode ---------------------------------------------------
bf_status bf_vertex_normals(uint32_t n_vertices, const float *positions, uint32_t n_faces, const uint32_t *indices, float *normals_out) {
    if ((n_vertices && (!positions || !normals_out)) || (n_faces && !indices)) return fail(BF_ERR_INVALID, "bf_vertex_normals: null array");
    for (size_t i = 0; i < 3 * (size_t) n_faces; ++i)
        if (indices[i] >= n_vertices)
            return fail(BF_ERR_INVALID, "bf_vertex_normals: face %zu names vertex %u of %u", i / 3, indices[i], n_vertices);
    bfk_host_vertex_normals(n_vertices, positions, n_faces, indices, normals_out);
    return BF_OK;
}

bf_status bf_scene_set_normal_mode(bf_scene *scene, uint32_t shape, uint32_t mode) {
    const char *fn = "bf_scene_set_normal_mode:";
    if (!scene) return fail(BF_ERR_INVALID, "%s null scene", fn);
    if (mode != BF_NORMALS_GIVEN && mode != BF_NORMALS_RECOMPUTE)
        return fail(BF_ERR_INVALID, "%s shape %u: unknown mode %u (BF_NORMALS_GIVEN or BF_NORMALS_RECOMPUTE)", fn, shape, mode);
    const bf_geometry::MeshTopo *tp = nullptr;
    const bf_status st = check_deform_shape(scene, shape, true, fn, &tp);
    if (st != BF_OK) return st;
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    if (m.normal_mode.size() < scene->info.n_shapes) m.normal_mode.resize(scene->info.n_shapes, (uint8_t) BF_NORMALS_GIVEN);
    m.normal_mode[shape] = (uint8_t) mode;      // read by the next position update; nothing moves now
    return BF_OK;
}

bf_status bf_scene_get_normal_mode(const bf_scene *scene, uint32_t shape, uint32_t *mode_out) {
    const char *fn = "bf_scene_get_normal_mode:";
    if (!scene || !mode_out) return fail(BF_ERR_INVALID, "%s null argument", fn);
    if (shape >= scene->info.n_shapes) return fail(BF_ERR_INVALID, "%s shape %u: the scene has %u shapes", fn, shape, scene->info.n_shapes);
    if (scene->ends.shapes_host[shape].type != BF_SHAPE_MESH) return fail(BF_ERR_INVALID, "%s shape %u is not a mesh", fn, shape);
    BF_ENTER(scene);
    *mode_out = scene->mesh.recomputes(shape) ? BF_NORMALS_RECOMPUTE : BF_NORMALS_GIVEN;
    return BF_OK;
}

// ---- velocity modes and the explicit field (bf_velocity.h) ------------------------------------------------------------
// what the four entries refuse first: `fn` ends in ':'
static bf_status check_velocity_shape(const bf_scene *scene, uint32_t shape, const char *fn) {
    if (!scene) return fail(BF_ERR_INVALID, "%s null scene", fn);
    if (shape >= scene->info.n_shapes) return fail(BF_ERR_INVALID, "%s shape %u: the scene has %u shapes", fn, shape, scene->info.n_shapes);
    if (scene->ends.shapes_host[shape].type != BF_SHAPE_MESH) return fail(BF_ERR_INVALID, "%s shape %u is not a mesh", fn, shape);
    return BF_OK;
}
// bf_scene_set_vertex_velocities and its device form behind their checks: the field (nullptr: zeros) gathered to the shape's slots
static bf_status gather_velocities(bf_scene *scene, uint32_t shape, const float *field_dev, hipStream_t stream) {
    MeshState &m = scene->mesh;
    bf_status st = BF_OK;
    if (field_dev && (st = deform_prepare(scene, stream)) != BF_OK) return st;      // the corner table
    HIP_TRY(bfk_launch_velocity_gather(scene->geom->corners, scene->d.tris, field_dev, shape, m.vel, scene->d.n_tris, stream));
    return BF_OK;
}

bf_status bf_scene_set_velocity_mode(bf_scene *scene, uint32_t shape, uint32_t mode, float dt) {
    const char *fn = "bf_scene_set_velocity_mode:";
    bf_status st = check_velocity_shape(scene, shape, fn);
    if (st != BF_OK) return st;
    if (mode != BF_VELOCITY_TWIST && mode != BF_VELOCITY_VERTEX && mode != BF_VELOCITY_DIFFERENCE)
        return fail(BF_ERR_INVALID, "%s shape %u: unknown mode %u (BF_VELOCITY_TWIST, BF_VELOCITY_VERTEX or BF_VELOCITY_DIFFERENCE)", fn, shape, mode);
    if (mode == BF_VELOCITY_DIFFERENCE && !(std::isfinite(dt) && dt > 0.f))
        return fail(BF_ERR_INVALID, "%s shape %u: dt = %g: the time step of BF_VELOCITY_DIFFERENCE must be finite and positive", fn, shape, (double) dt);
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    const uint32_t n_shapes = scene->info.n_shapes;
    if (mode == BF_VELOCITY_TWIST && !m.vel) return BF_OK;      // no shape has left the default yet
    // the call has no stream: it waits for the handle's work in flight (an open rolling sequence ends, as for a class table), changes
    // the tables, and is complete when it returns
    if ((st = close_sequence(scene, scene->run.roll.stream)) != BF_OK) return st;
    HIP_TRY(scene->run.last.wait());
    if (!m.vel) {
        // everything exists before any state changes: a failed call leaves the scene as it was
        const size_t vel_bytes = (size_t) scene->d.n_tris * bfvel::kRowsPerSlot * sizeof(float4), tab_bytes = (size_t) n_shapes * sizeof(float2);
        float4 *vel = nullptr;
        float2 *tab = nullptr;
        hipError_t he = hipMalloc((void **) &vel, vel_bytes);
        if (he == hipSuccess) he = hipMalloc((void **) &tab, tab_bytes);
        if (he == hipSuccess) he = hipMemset(vel, 0, vel_bytes);
        if (he != hipSuccess) {
            (void) hipGetLastError();
            if (vel) (void) hipFree(vel);
            if (tab) (void) hipFree(tab);
            return fail(BF_ERR_NOMEM, "%s hipMalloc(%zu bytes) for the velocity rows: %s", fn, vel_bytes + tab_bytes, hipGetErrorString(he));
        }
        m.vel = vel;
        m.vel_tab = tab;
    }
    if (m.vel_mode.size() < n_shapes) m.vel_mode.resize(n_shapes, (uint8_t) BF_VELOCITY_TWIST);
    if (m.vel_dt.size() < n_shapes) m.vel_dt.resize(n_shapes, 0.f);
    m.vel_mode[shape] = (uint8_t) mode;
    m.vel_dt[shape] = mode == BF_VELOCITY_DIFFERENCE ? dt : 0.f;
    std::vector<float2> tab(n_shapes);
    for (uint32_t k = 0; k < n_shapes; ++k) {
        const uint32_t bits = m.vel_mode[k];
        std::memcpy(&tab[k].x, &bits, 4);
        tab[k].y = m.vel_dt[k];
    }
    HIP_TRY(hipMemcpy(m.vel_tab, tab.data(), tab.size() * sizeof(float2), hipMemcpyHostToDevice));
    // the field is zero until one is given (BF_VELOCITY_VERTEX) or a move differences it (BF_VELOCITY_DIFFERENCE)
    if (mode != BF_VELOCITY_TWIST && (st = gather_velocities(scene, shape, nullptr, nullptr)) != BF_OK) return st;
    if ((st = velocity_stamp(scene, m.vel, nullptr)) != BF_OK) return st;
    HIP_TRY(hipStreamSynchronize(nullptr));
    return BF_OK;
}

bf_status bf_scene_get_velocity_mode(const bf_scene *scene, uint32_t shape, uint32_t *mode_out, float *dt_out) {
    const char *fn = "bf_scene_get_velocity_mode:";
    const bf_status st = check_velocity_shape(scene, shape, fn);
    if (st != BF_OK) return st;
    if (!mode_out && !dt_out) return fail(BF_ERR_INVALID, "%s null argument", fn);
    BF_ENTER(scene);
    if (mode_out) *mode_out = scene->mesh.velocity_mode(shape);
    if (dt_out) *dt_out = shape < scene->mesh.vel_dt.size() ? scene->mesh.vel_dt[shape] : 0.f;
    return BF_OK;
}

bf_status bf_scene_set_vertex_velocities(bf_scene *scene, uint32_t shape, const float *vel, void *stream_) {
    const char *fn = "bf_scene_set_vertex_velocities:";
    bf_status st = check_velocity_shape(scene, shape, fn);
    if (st != BF_OK) return st;
    const size_t n = 3 * (size_t) scene->geom->topo[shape].n_vertices;
    for (size_t i = 0; vel && i < n; ++i)
        if (!std::isfinite(vel[i])) return fail(BF_ERR_INVALID, "%s shape %u: non-finite value at vertex %zu", fn, shape, i / 3);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    if (m.velocity_mode(shape) != BF_VELOCITY_VERTEX || !m.vel)
        return fail(BF_ERR_INVALID, "%s shape %u is not in BF_VELOCITY_VERTEX (bf_scene_set_velocity_mode)", fn, shape);
    if ((st = mesh_enter(scene, stream)) != BF_OK) return st;
    if (!vel || n == 0) return (st = gather_velocities(scene, shape, nullptr, stream)) != BF_OK ? st : mark_last(scene, stream);
    // the caller's array through the handle's upload buffer, as a vertex update's
    const size_t bytes = n * sizeof(float);
    if (m.vtx_ev) HIP_TRY(hipEventSynchronize(m.vtx_ev));      // the previous gather may still read it
    if (m.vtx_cap < bytes) {
        if (m.vtx_host) (void) hipHostFree(m.vtx_host);
        if (m.vtx_dev) (void) hipFree(m.vtx_dev);
        m.vtx_host = m.vtx_dev = nullptr;
        m.vtx_cap = 0;
        HIP_TRY(hipHostMalloc(&m.vtx_host, bytes));
        HIP_TRY(hipMalloc(&m.vtx_dev, bytes));
        m.vtx_cap = bytes;
    }
    if (!m.vtx_ev) HIP_TRY(hipEventCreateWithFlags(&m.vtx_ev, hipEventDisableTiming));
    std::memcpy(m.vtx_host, vel, bytes);
    HIP_TRY(hipMemcpyAsync(m.vtx_dev, m.vtx_host, bytes, hipMemcpyHostToDevice, stream));
    st = gather_velocities(scene, shape, (const float *) m.vtx_dev, stream);
    HIP_TRY(hipEventRecord(m.vtx_ev, stream));
    if (st != BF_OK) return st;
    return mark_last(scene, stream);
}

bf_status bf_scene_set_vertex_velocities_device(bf_scene *scene, uint32_t shape, const float *vel_dev, void *stream_) {
    const char *fn = "bf_scene_set_vertex_velocities_device:";
    bf_status st = check_velocity_shape(scene, shape, fn);
    if (st != BF_OK) return st;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    if (m.velocity_mode(shape) != BF_VELOCITY_VERTEX || !m.vel)
        return fail(BF_ERR_INVALID, "%s shape %u is not in BF_VELOCITY_VERTEX (bf_scene_set_velocity_mode)", fn, shape);
    if ((st = mesh_enter(scene, stream)) != BF_OK) return st;
    if ((st = gather_velocities(scene, shape, scene->geom->topo[shape].n_vertices ? vel_dev : nullptr, stream)) != BF_OK) return st;
    return mark_last(scene, stream);
}

// ---- rebuild of both trees on the device (bf_build.hip) ---------------------------------------------------------------
/* test hook (not part of the ABI): nth > 0: the builder's nth device allocation fails; nth < 0: the |nth|-th allocation of the
   rebuild's own arrays fails; 0: off */
bf_status bfdbg_rebuild_fail_alloc(int nth) {
    bfk_build_fail_alloc(nth > 0 ? nth : 0);
    g_rebuild_fail_alloc = nth < 0 ? -nth : 0;
    return BF_OK;
}

bf_status bf_scene_rebuild_bvh(bf_scene *scene, void *stream_) {
    if (!scene) return fail(BF_ERR_INVALID, "bf_scene_rebuild_bvh: null scene");
    if (scene->d.n_tris == 0) return BF_OK;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    MeshState &m = scene->mesh;
    bf_status st = mesh_enter(scene, stream);
    if (st != BF_OK) return st;
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t n = scene->d.n_tris;
    const bool want_wide = scene->d.wnodes != nullptr, want_quant = scene->d.qnodes != nullptr, posed = m.tris0 != nullptr;
    bfk_build_in bin = {scene->d.tris, n, m.origin_scale_built, want_wide ? 1 : 0, stream};
    bfk_build_out bo;
    {
        char text[384];
        text[0] = 0;
        const int bst = bfk_build_bvh(&bin, &bo, text, sizeof(text));
        if (bst) return fail(bst == 1 ? BF_ERR_NOMEM : (bst == 3 ? BF_ERR_UNSUPPORTED : BF_ERR_DEVICE), "bf_scene_rebuild_bvh: %s", text);
    }
    // everything the new tree needs is allocated and filled before the handle changes: a failure frees it and leaves the scene as it was
    std::vector<void *> fresh = {bo.nodes, bo.wnodes};
    auto drop = [&]() {
        for (void *p : fresh)
            if (p) (void) hipFree(p);
        if (bo.order) (void) hipFree(bo.order);
    };
    if (want_wide && 16u * std::max(1u, bo.depth16) > (uint32_t) bfd::kWideStack) {
        drop();
        return fail(BF_ERR_UNSUPPORTED, "bf_scene_rebuild_bvh: the rebuilt sixteen-wide tree is %u levels deep: its row stack (%u entries) "
                                        "exceeds %d", bo.depth16, 16u * bo.depth16, bfd::kWideStack);
    }
    // The sixteen-wide array is sized with one node MORE than everywhere else: the builder's array (bf_build.hip) carries the zeroed
    // padding node a row's speculative load may touch, it becomes d.wnodes as it is, and wnodes0 is a whole copy of it.  The copies
    // own_geometry and the batches make hold the n_wnodes nodes the refit kernels read and write.
    const MeshState::Bytes B = MeshState::bytes(n, bo.n_nodes, want_wide ? (size_t) bo.n_wnodes + 1 : 0);
    const size_t tri_rows = (size_t) n * bfd::kTriStride;
    const float4 *old_normals0 = m.normals0 && m.normals0 != scene->d.normals ? m.normals0 : nullptr;
    float4 *tris = nullptr, *tris0 = nullptr, *normals = nullptr, *normals0 = nullptr, *uvs = nullptr, *corners = nullptr, *qnodes = nullptr;
    float4 *nodes0 = nullptr, *wnodes0 = nullptr, *spill = nullptr;
    // (the order and the number of these allocations are what bfdbg_rebuild_fail_alloc counts)
    DevAlloc alloc{fresh, "bf_scene_rebuild_bvh", g_rebuild_fail_alloc};
    auto take = [&](bool wanted, size_t bytes, float4 **out) {
        if (wanted && st == BF_OK) st = alloc(bytes, out);
    };
    take(true, B.tris, &tris);
    take(posed, B.tris, &tris0);
    take(scene->d.normals != nullptr, B.normals, &normals);
    take(old_normals0 != nullptr, B.normals, &normals0);
    take(scene->d.uvs != nullptr, 3 * (size_t) n * sizeof(float4), &uvs);      // three rows per triangle, n apart (bf_device.h)
    take(scene->geom->corners != nullptr, (size_t) n * sizeof(uint4), &corners);
    take(want_quant && bo.n_nodes, B.nodes / 2, &qnodes);
    take(posed && B.nodes, B.nodes, &nodes0);
    take(posed && B.wnodes, B.wnodes, &wnodes0);
    const uint32_t old_spill = scene->d.stack_need > 16 ? scene->d.stack_need - 16 : 1, new_spill = bo.stack4 > 16 ? bo.stack4 - 16 : 1;
    take(new_spill > old_spill, (size_t) scene->d.spill_stride * new_spill * sizeof(int), &spill);
    float4 *vel = nullptr;      // the velocity rows follow the slots (bf_scene_set_velocity_mode); the handle's own, like the spill columns
    take(m.vel != nullptr, (size_t) n * bfvel::kRowsPerSlot * sizeof(float4), &vel);
    if (st != BF_OK) {
        drop();
        return st;
    }
    auto enqueue = [&]() -> hipError_t {
        hipError_t e = bfk_build_gather(bo.order, n, scene->d.tris, tris, bfd::kTriStride, stream);
        if (e == hipSuccess) e = hipMemsetAsync(tris + tri_rows, 0, kTriPad * sizeof(float4), stream);
        if (e == hipSuccess && tris0) e = bfk_build_gather(bo.order, n, m.tris0, tris0, bfd::kTriStride, stream);
        if (e == hipSuccess && tris0) e = hipMemsetAsync(tris0 + tri_rows, 0, kTriPad * sizeof(float4), stream);
        if (e == hipSuccess && normals) e = bfk_build_gather(bo.order, n, scene->d.normals, normals, 3, stream);
        if (e == hipSuccess && normals0) e = bfk_build_gather(bo.order, n, old_normals0, normals0, 3, stream);
        for (size_t part = 0; part < 3; ++part)
            if (e == hipSuccess && uvs) e = bfk_build_gather(bo.order, n, scene->d.uvs + part * n, uvs + part * n, 1, stream);
        if (e == hipSuccess && corners) e = bfk_build_gather(bo.order, n, (const float4 *) scene->geom->corners, corners, 1, stream);
        if (e == hipSuccess && vel) e = bfk_build_gather(bo.order, n, m.vel, vel, bfvel::kRowsPerSlot, stream);
        // the quantised copies by the refit's own kernel (no levels to re-fit: the boxes are the builder's)
        const uint32_t no_levels[1] = {0u};
        if (e == hipSuccess && qnodes)
            e = bfk_launch_refit(tris, bo.nodes, bo.nodes, qnodes, bo.n_nodes, nullptr, no_levels, 0u, nullptr, nullptr, nullptr, nullptr, no_levels, 0u,
                                 nullptr, 0.f, 1u, 0u, stream);
        if (e == hipSuccess && nodes0) e = hipMemcpyAsync(nodes0, bo.nodes, B.nodes, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess && wnodes0) e = hipMemcpyAsync(wnodes0, bo.wnodes, B.wnodes, hipMemcpyDeviceToDevice, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        return e;
    };
    {
        const hipError_t e = enqueue();
        if (e != hipSuccess) {
            drop();
            return fail(BF_ERR_DEVICE, "bf_scene_rebuild_bvh: %s", hipGetErrorString(e));
        }
    }
    (void) hipFree(bo.order);
    bo.order = nullptr;

    // the swap.  The new arrays belong to a geometry object of the handle's own (copy on write: clones keep the old one alive and
    // unchanged; a clone taken from now on shares the new one as it would share a created scene's)
    auto g2 = std::make_shared<bf_geometry>();
    g2->topo = scene->geom->topo;
    g2->corners = (uint4 *) corners;
    g2->normal_index = scene->geom->normal_index;      // per vertex and face, not per slot: shared as they are
    for (void *p : fresh)
        if (p && p != spill && p != vel) g2->owned.push_back(p);
    const MeshState::Refit &rf = m.refit;
    const void *gone[] = {m.tris0, m.nodes0, m.wnodes0, scene->d.tris, scene->d.nodes, scene->d.wnodes, scene->d.qnodes, scene->d.normals,
                          m.normals0, rf.lvl4, rf.lvl16, rf.ubox4, rf.ubox16, spill ? scene->d.spill : nullptr};
    for (const void *p : gone) {      // those that are the handle's own go now (the shared geometry's go with its last user)
        const auto it = std::find(scene->owned.begin(), scene->owned.end(), p);
        if (!p || it == scene->owned.end()) continue;
        (void) hipFree(*it);
        scene->owned.erase(it);
    }
    scene->geom = g2;
    scene->geom_token = std::make_shared<char>(0);
    bfd::DScene &d = scene->d;
    d.tris = tris;
    d.nodes = bo.nodes;
    d.qnodes = qnodes;
    d.wnodes = want_wide ? bo.wnodes : nullptr;
    d.normals = normals;
    d.uvs = uvs;
    d.n_nodes = bo.n_nodes;
    d.root = bo.root;
    d.wroot = want_wide ? bo.wroot : bfd_no_node();
    d.n_wnodes = want_wide ? bo.n_wnodes : 0u;
    if (want_wide) {
        uint32_t rlog = 2;
        while (rlog > 0 && (16u << rlog) * std::max(1u, bo.depth16) > (uint32_t) bfd::kWideStack) --rlog;
        if (scene->tun.wide_rows_log >= 0) rlog = std::min<uint32_t>(rlog, (uint32_t) scene->tun.wide_rows_log);
        d.wrows_log = rlog;
    }
    d.stack_need = bo.stack4;
    if (spill) {
        d.spill = (int *) spill;
        scene->owned.push_back(spill);
    }
    m.reset_after_rebuild(tris0, posed ? nodes0 : nullptr, posed ? wnodes0 : nullptr, normals0);
    if (vel) {
        (void) hipFree(m.vel);      // (the gather has run: enqueue() waited for the stream)
        m.vel = vel;
    }
    float oscale = m.origin_scale_built;
    for (int k = 0; k < 3; ++k) oscale = std::max({oscale, std::fabs(bo.lo[k]), std::fabs(bo.hi[k])});
    m.origin_scale_built = oscale;      // (what the builder padded for: kept, never lowered)
    bf_scene_info &inf = scene->info;
    inf.n_bvh_nodes = bo.n_nodes;
    inf.bvh_depth = bo.depth4;
    inf.bvh_stack_need = bo.stack4;
    {
        float mx = 0.f;
        for (int k = 0; k < 3; ++k) mx = std::max({mx, bo.hi[k] - bo.lo[k], std::fabs(bo.lo[k]), std::fabs(bo.hi[k])});
        const float e = 2e-6f * mx + 2e-7f * oscale + 1e-30f;
        for (int k = 0; k < 3; ++k) inf.bbox_min[k] = bo.lo[k] - e, inf.bbox_max[k] = bo.hi[k] + e;
    }
    if (vel && (st = velocity_stamp(scene, m.vel, stream)) != BF_OK) return st;      // a range-rate table names the rows it reads
    return mark_last(scene, stream);
}

// ---- batches of geometry versions ------------------------------------------------------------------------------------
// Render k reads geometry version k: the base rows moved by to_world[k] and both trees re-fitted, by bf_scene_transform_meshes' kernels,
// for all renders of a chunk at once (grid y = version).  The handle's own geometry, pose, padding bound and clones are not touched.
bf_status bf_render_motion_batch_device(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_shapes,
                                        const float *to_world, float *hist_dev, bf_path_record *records_dev, void *stream_, bf_stats *stats_out) {
    const char *fn = "bf_render_motion_batch_device:";
    if (!to_world) return fail(BF_ERR_INVALID, "%s null argument", fn);
    bf_status st = check_batch_call(fn, "motion", scene, launch, n_renders, to_world, n_shapes, hist_dev);
    if (st != BF_OK) return st;
    // every render's table is checked before anything is enqueued: a failed call leaves the scene as it was
    std::vector<uint8_t> moves((size_t) n_renders * n_shapes, 0);
    if ((st = check_rigid_tables(scene, fn, n_renders, n_shapes, to_world, moves.data())) != BF_OK) return st;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    if (batch_ends_early(scene, launch, n_renders, seeds, hist_dev, records_dev, stream_, stats_out, &st)) return st;
    MeshState &m = scene->mesh;
    if ((st = mesh_enter(scene, stream)) != BF_OK) return st;
    if (!m.refit.ready && (st = refit_prepare(scene, stream)) != BF_OK) return st;
    // one padding bound for every version of the call: the handle's, raised to cover all moved meshes of all renders
    float oscale = m.origin_scale_built;
    for (uint32_t k = 0; k < n_renders; ++k)
        oscale = origin_bound(m.refit.mesh_box, n_shapes, to_world + (size_t) 12 * n_shapes * k, 12, moves.data() + (size_t) n_shapes * k, oscale);
    return render_versions(scene, launch, n_renders, seeds, hist_dev, records_dev, stream_, stats_out, "bf_render_motion_batch_device",
                           [&](uint32_t k0, uint32_t kc, float4 *a, const MotionLayout &L) -> bf_status {
        // the chunk's transform tables
        const size_t n = (size_t) kc * n_shapes, bytes = n * 16 * sizeof(float);
        bf_scene::Stage *stg = nullptr;
        bf_status pst = stage_acquire(scene, bytes, &stg);
        if (pst != BF_OK) return pst;
        pack_rigid((float *) stg->host, to_world + 12 * (size_t) k0 * n_shapes, moves.data() + (size_t) k0 * n_shapes, n);
        if ((pst = stage_commit(stg, bytes, stream)) != BF_OK) return pst;
        HIP_TRY(launch_rigid(scene, m.base(scene->d).normals, (const float *) stg->dev, n_shapes * 16u, oscale, arena_dst(scene, a, L, kc), stream));
        return BF_OK;
    });
}

// bf_render_deform_batch_device: the motion batch with a vertex gather in front.  Version k = the deforming shapes from slice k of
// their arrays, every other mesh from the handle's base rows, then to_world[k] (absolute; NULL: none), in ONE pass over the rows
// (bf_deform_tris_kernel applies rigid_apply to what it gathered: the arithmetic of an update followed by a transform call), then
// the level kernels with the version dimension.  Arena, chunking and rendering as the motion batch.
bf_status bf_render_deform_batch_device(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_deform,
                                        const uint32_t *shapes, const float *const *positions_dev, const float *const *normals_dev, float bound,
                                        uint32_t n_shapes, const float *to_world, float *hist_dev, bf_path_record *records_dev, void *stream_,
                                        bf_stats *stats_out) {
    const char *fn = "bf_render_deform_batch_device:";
    if (n_deform && (!shapes || !positions_dev)) return fail(BF_ERR_INVALID, "%s null argument", fn);
    bf_status st = check_batch_call(fn, "deform", scene, launch, n_renders, to_world, n_shapes, hist_dev);
    if (st != BF_OK) return st;
    if (n_deform && (!(bound > 0.f) || !std::isfinite(bound))) return fail(BF_ERR_INVALID, "%s bound must be positive and finite", fn);
    n_shapes = scene->info.n_shapes;
    std::vector<bfd::DDeformSrc> src(n_shapes);
    std::memset(src.data(), 0, src.size() * sizeof(bfd::DDeformSrc));
    for (uint32_t j = 0; j < n_deform; ++j) {
        const bf_geometry::MeshTopo *tp = nullptr;
        const float *nj = normals_dev ? normals_dev[j] : nullptr;
        bf_status cst = check_deform_shape(scene, shapes[j], nj != nullptr, fn, &tp);
        if (cst != BF_OK) return cst;
        if (!positions_dev[j]) return fail(BF_ERR_INVALID, "%s shape %u: null positions", fn, shapes[j]);
        if (src[shapes[j]].pos) return fail(BF_ERR_INVALID, "%s shape %u is listed twice", fn, shapes[j]);
        src[shapes[j]].pos = positions_dev[j];
        src[shapes[j]].nrm = nj;
        src[shapes[j]].nv = tp->n_vertices;
    }
    std::vector<uint8_t> moves(to_world ? (size_t) n_renders * n_shapes : 0, 0);
    if (to_world && (st = check_rigid_tables(scene, fn, n_renders, n_shapes, to_world, moves.data())) != BF_OK) return st;
    BF_ENTER(scene);
    if (batch_ends_early(scene, launch, n_renders, seeds, hist_dev, records_dev, stream_, stats_out, &st)) return st;
    return deform_versions(scene, launch, n_renders, seeds, src, bound, to_world, moves, hist_dev, records_dev, stream_, stats_out,
                           "bf_render_deform_batch_device", [&](uint32_t k0, uint32_t, bfd::DDeformSrc *hs) -> bf_status {
        // the sources advanced to slice k0
        for (uint32_t k = 0; k < n_shapes; ++k) {
            if (hs[k].pos) hs[k].pos += (size_t) k0 * 3 * hs[k].nv;
            if (hs[k].nrm) hs[k].nrm += (size_t) k0 * 3 * hs[k].nv;
        }
        return BF_OK;
    });
}

/* test hook (not part of the ABI): the ray-origin bound the handle's boxes are padded for (bf_bvh.h) */
bf_status bfdbg_scene_origin_scale(const bf_scene *scene, float *out) {
    if (!scene || !out) return fail(BF_ERR_INVALID, "bfdbg_scene_origin_scale: null argument");
    *out = scene->mesh.origin_scale_built;
    return BF_OK;
}

/* test hook (not part of the ABI): what the device wrote, read back.  which = 4 / 16: the Node4 / Node16 array; 64: the Node4Q
   array (BF_ERR_UNSUPPORTED unless the scene was created under BF_QUANT_BVH=1).  version = -1: the handle's own arrays; k >= 0:
   geometry version k of the handle's last motion / deform batch, from the arena (BF_ERR_INVALID if that batch was chunked or k
   is out of range).  nodes_out (`bytes` of it, at least the array's size; a call with too few fails with the text "needs <n>
   bytes", as bf_scene_read_bvh), rows_out (float4[n_triangles][3]) and normals_out (float4[n_triangles][3], the posed vertex
   normals; left alone if the scene has none) may each be NULL.  Finishes the open sequence and waits for the handle's last work. */
bf_status bfdbg_scene_read_tree(const bf_scene *scene, uint32_t which, int32_t version, void *nodes_out, uint64_t bytes, float *rows_out,
                                float *normals_out) {
    if (!scene) return fail(BF_ERR_INVALID, "bfdbg_scene_read_tree: null scene");
    if (which != 4u && which != 16u && which != 64u) return fail(BF_ERR_INVALID, "bfdbg_scene_read_tree: which = %u (4, 16 or 64)", which);
    BF_ENTER(scene);
    {
        bf_status cst = close_sequence(scene, scene->run.roll.stream);
        if (cst != BF_OK) return cst;
    }
    HIP_TRY(scene->run.last.wait());
    const bfd::DScene &d = scene->d;
    const MeshState &m = scene->mesh;
    if (which == 16u && !d.wnodes) return fail(BF_ERR_UNSUPPORTED, "bfdbg_scene_read_tree: the scene has no sixteen-wide tree");
    if (which == 64u && !d.qnodes) return fail(BF_ERR_UNSUPPORTED, "bfdbg_scene_read_tree: the scene has no quantised nodes (BF_QUANT_BVH=1)");
    const float4 *tris = d.tris, *normals = d.normals, *nodes = d.nodes, *wnodes = d.wnodes, *qnodes = d.qnodes;
    if (version >= 0) {
        const MotionLayout L = motion_layout(d, m.batch_vel);
        if (!m.arena || (uint32_t) version >= m.batch_versions || L.rows != m.batch_rows)
            return fail(BF_ERR_INVALID, "bfdbg_scene_read_tree: version %d: the handle's last batch left %u whole versions in its arena "
                                        "(none if it was chunked)", version, m.batch_versions);
        const RefitDst o = arena_dst(scene, m.arena + (size_t) version * L.rows, L, 1u);
        tris = o.tris, normals = o.normals, nodes = o.nodes, wnodes = o.wnodes, qnodes = o.qnodes;
    } else if (version != -1) {
        return fail(BF_ERR_INVALID, "bfdbg_scene_read_tree: version %d", version);
    }
    const uint64_t need = which == 4u ? (uint64_t) d.n_nodes * sizeof(bf::Node4)
                        : which == 16u ? (uint64_t) d.n_wnodes * sizeof(bf::Node16) : (uint64_t) d.n_nodes * sizeof(bf::Node4Q);
    if (nodes_out || bytes) {
        if (bytes < need || (need && !nodes_out))
            return fail(BF_ERR_INVALID, "bfdbg_scene_read_tree: nodes_out needs %llu bytes (%llu given)", (unsigned long long) need,
                        (unsigned long long) bytes);
        if (need) HIP_TRY(hipMemcpy(nodes_out, which == 4u ? nodes : (which == 16u ? wnodes : qnodes), need, hipMemcpyDeviceToHost));
    }
    const size_t row_bytes = (size_t) d.n_tris * 3 * sizeof(float4);
    static_assert(bfd::kTriStride == 3, "rows_out is float4[n_triangles][3]");
    if (rows_out && d.n_tris) HIP_TRY(hipMemcpy(rows_out, tris, row_bytes, hipMemcpyDeviceToHost));
    if (normals_out && normals && d.n_tris) HIP_TRY(hipMemcpy(normals_out, normals, row_bytes, hipMemcpyDeviceToHost));
    return BF_OK;
}

}  // extern "C"
