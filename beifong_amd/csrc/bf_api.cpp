// C ABI of libbeifong_hip.so (include/beifong_hip.h): handle lifetime, BVH
// build, device upload, queries and the multi-GPU entry points.  Plain pointers and sizes in,
// integer status out; no exceptions cross the boundary.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <limits>
#include <new>
#include <string>

#include <dlfcn.h>
// RCCL is dlopen'ed on first use (bf_allreduce_device); only the handful of types and prototypes below are needed, so a ROCm
// install without the RCCL development headers still builds the core (the values are rccl.h's: ncclSuccess 0, ncclFloat32 7,
// ncclSum 0)
#if defined(__has_include) && __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm *ncclComm_t;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclFloat = 7 } ncclDataType_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
ncclResult_t ncclCommInitAll(ncclComm_t *comm, int ndev, const int *devlist);
ncclResult_t ncclCommDestroy(ncclComm_t comm);
ncclResult_t ncclAllReduce(const void *sendbuff, void *recvbuff, size_t count, ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm,
                           hipStream_t stream);
ncclResult_t ncclGroupStart(void);
ncclResult_t ncclGroupEnd(void);
const char *ncclGetErrorString(ncclResult_t result);
}
#endif

#include <map>
#include <mutex>

#include "bf_scene.h"
#include "bf_sum.h"


static thread_local std::string g_err;

bf_status fail(bf_status st, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return st;
}

namespace {
template <typename T> bf_status upload(const std::vector<T> &v, const T **out, std::vector<void *> &owned, uint64_t &bytes) {
    *out = nullptr;
    if (v.empty()) return BF_OK;
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, v.size() * sizeof(T)));
    owned.push_back(p);
    HIP_TRY(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    bytes += v.size() * sizeof(T);
    *out = reinterpret_cast<const T *>(p);
    return BF_OK;
}
}  // namespace

static bf_tunables read_tunables() {
    bf_tunables t;
    auto num = [](const char *name, long long dflt) -> long long {
        const char *e = getenv(name);
        return e ? strtoll(e, nullptr, 10) : dflt;
    };
    t.pool = (uint32_t) std::max<long long>(1024, std::min<long long>(num("BF_WF_POOL", 1ll << 24), 1ll << 26));
    t.tail = num("BF_WF_TAIL", -1);
    t.trace_refill = (uint32_t) num("BF_TRACE_REFILL", bfd::kTraceRefill);
    t.trace_stragglers = (uint32_t) num("BF_TRACE_STRAGGLERS", bfd::kTraceStragglers);
    t.shade_chain = (uint32_t) std::max<long long>(1, num("BF_SHADE_CHAIN", bfd::kShadeChain));
    t.row_jobs = (uint32_t) num("BF_TAIL_ROWJOBS", bfd::kTailRowJobs);
    t.shade_waves = (int) std::max<long long>(1, std::min<long long>(4, num("BF_SHADE_WAVES", 3)));
    if (getenv("BF_SHADE_WAVES")) t.gen_waves = t.shade_waves;      // an explicit budget is every shading launch's
    {
        const long long w = num("BF_TRACE_WAVES", 5);
        t.trace_waves = w < 5 ? 4 : (w > 5 ? 6 : 5);
    }
    t.tail_waves = num("BF_TAIL_WAVES", 3) == 2 ? 2 : 3;
    t.tail_spread = (unsigned) std::max<long long>(1, num("BF_TAIL_SPREAD", 1));
    t.tail_blocks = (unsigned) std::max<long long>(0, num("BF_TAIL_BLOCKS", 0));
    t.tail_share = (int) num("BF_TAIL_SHARE", -1);
    t.allow_plan = num("BF_WF_SYNC", 0) == 0;
    t.roll_iters = (uint32_t) std::max<long long>(0, std::min<long long>(32, num("BF_ROLL_ITERS", 0)));
    t.roll_live = (uint32_t) std::max<long long>(0, std::min<long long>(num("BF_ROLL_LIVE", 0), 1ll << 30));
    t.no_wide = getenv("BF_NO_WIDE_BVH") != nullptr;
    t.quant = num("BF_QUANT_BVH", 0) != 0;
    t.wide_rows_log = (int) num("BF_WIDE_ROWS_LOG", -1);
    t.lean = num("BF_LEAN", 1) != 0;
    t.tab_cache = num("BF_TAB_CACHE", 1) != 0;
    t.shade_split = num("BF_SHADE_SPLIT", 0) != 0;
    t.chain_min = (uint32_t) std::max<long long>(0, std::min<long long>(num("BF_CHAIN_MIN", 16), 64));
    t.grid_share = (uint32_t) std::max<long long>(0, std::min<long long>(num("BF_GRID_SHARE", 3), 16));
    t.grid_small = (uint32_t) std::max<long long>(0, std::min<long long>(num("BF_GRID_SMALL", 1ll << 22), 1ll << 30));
    t.roll_join = num("BF_ROLL_JOIN", 1) != 0;
    t.debug_surv_batches = (uint32_t) std::max<long long>(0, std::min<long long>(num("BF_DEBUG_SURV_BATCHES", 0), 1 << 14));
    return t;
}

extern "C" {

int bf_version(void) { return BF_ABI_VERSION; }
uint32_t bf_abi_sizeof(uint32_t which) {
    static const uint32_t sizes[BF_ABI_STRUCTS] = {sizeof(bf_material), sizeof(bf_shape), sizeof(bf_emitter), sizeof(bf_sensor),
                                                   sizeof(bf_scene_desc), sizeof(bf_launch), sizeof(bf_path_record), sizeof(bf_stats),
                                                   sizeof(bf_scene_info), sizeof(bf_batch)};
    return which < BF_ABI_STRUCTS ? sizes[which] : 0u;
}
uint64_t bf_abi_fingerprint(void) { return BF_ABI_FINGERPRINT; }
const char *bf_last_error(void) { return g_err.c_str(); }

int bf_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

bf_status bf_set_device(int device) {
    HIP_TRY(hipSetDevice(device));
    return BF_OK;
}

static uint32_t film_pixels(const bf_launch *lp) {
    return (lp->spp && lp->film_width && lp->film_height) ? lp->film_width * lp->film_height : 1u;
}

uint32_t bf_launch_channels(const bf_launch *lp) {
    if (!lp) return 0;
    if (lp->flags & BF_FLAG_MOMENT) {
        // beifong_hip.h, BF_FLAG_MOMENT: 5 + 2 (A + 3) channels per pixel (moment.cpp:39-52), m2_Y / m2_I m2_Q per ADC cell
        switch (lp->mode) {
            case BF_MODE_PATH: return 11 * film_pixels(lp);
            case BF_MODE_RANGE: return (11 + 2 * lp->bins) * film_pixels(lp);
            case BF_MODE_TIME: return (11 + 6 * lp->bins) * film_pixels(lp);
            case BF_MODE_RECEIVE_RAW: return (4 + lp->phase_bins) * lp->bins * lp->bins_y;
            case BF_MODE_RECEIVE_IQ: return 5 * lp->bins * lp->bins_y;
        }
        return 0;
    }
    switch (lp->mode) {
        case BF_MODE_PATH: return 5 * film_pixels(lp);
        case BF_MODE_RANGE: return (5 + lp->bins) * film_pixels(lp);
        case BF_MODE_TIME: return (5 + 3 * lp->bins) * film_pixels(lp);
        case BF_MODE_RECEIVE_RAW: return (3 + lp->phase_bins) * lp->bins * lp->bins_y;
        case BF_MODE_RECEIVE_IQ: return 3 * lp->bins * lp->bins_y;
    }
    return 0;
}

uint32_t bf_scene_launch_channels(const bf_scene *scene, const bf_launch *lp) {
    const uint32_t n = bf_launch_channels(lp);
    if (scene && lp && (lp->flags & BF_FLAG_AOV) && scene->run.aov.n && lp->mode <= BF_MODE_TIME && !(lp->flags & (BF_FLAG_MOMENT | BF_FLAG_CLASSES))) {
        // beifong_hip.h, BF_FLAG_AOV: the table's K floats behind X Y Z A W, nested.R G B A last (aov.cpp:83-150)
        const uint64_t all = (uint64_t) n + (uint64_t) film_pixels(lp) * (bf_aov_floats(scene->run.aov.n, scene->run.aov.types) + 4u);
        return all > UINT32_MAX ? 0u : (uint32_t) all;
    }
    if (!scene || !lp || !(lp->flags & BF_FLAG_CLASSES)) return n;
    const uint64_t all = (uint64_t) n * std::max(1u, bfd::scene_n_classes(scene->d));
    return all > UINT32_MAX ? 0u : (uint32_t) all;      // (0: as for an unknown mode; check_launch refuses such a launch by name)
}

bf_status bf_scene_destroy(bf_scene *s) {
    if (!s) return BF_OK;
    // kernels of this handle that are still in flight read the arrays freed below (an open rolling sequence is simply
    // abandoned: its histograms stay incomplete, as documented)
    (void) s->run.last.wait();
    if (s->run.roll.open && s->peers_rolling) s->peers_rolling->fetch_sub(1, std::memory_order_relaxed);
    for (void *p : s->owned) (void) hipFree(p);
    for (auto &st : s->stage) {
        if (st.ev) {
            (void) hipEventSynchronize(st.ev);
            (void) hipEventDestroy(st.ev);
        }
        if (st.host) (void) hipHostFree(st.host);
        if (st.dev) (void) hipFree(st.dev);
    }
    delete s;      // (~RenderState, ~MeshState, ~EndpointState: what renders, moved meshes and the endpoint tables allocated)
    return BF_OK;
}

// Next staging slot with room for `bytes` (see bf_scene::Stage): *host is pinned memory the caller fills, *dev its
// device mirror; stage_commit() enqueues the copy and the slot's event.
bf_status stage_acquire(const bf_scene *sc, size_t bytes, bf_scene::Stage **out) {
    bf_scene::Stage &st = sc->stage[sc->stage_next];
    sc->stage_next = (sc->stage_next + 1) % bf_scene::kStageSlots;
    if (st.busy) {
        HIP_TRY(hipEventSynchronize(st.ev));
        st.busy = false;
    }
    if (st.cap < bytes) {
        if (st.host) (void) hipHostFree(st.host);
        if (st.dev) (void) hipFree(st.dev);
        st.host = st.dev = nullptr;
        st.cap = 0;
        const size_t cap = std::max<size_t>(4096, (bytes + 4095) & ~size_t(4095));
        HIP_TRY(hipHostMalloc(&st.host, cap));
        HIP_TRY(hipMalloc(&st.dev, cap));
        st.cap = cap;
    }
    if (!st.ev) HIP_TRY(hipEventCreateWithFlags(&st.ev, hipEventDisableTiming));
    *out = &st;
    return BF_OK;
}
bf_status stage_commit(bf_scene::Stage *st, size_t bytes, hipStream_t stream) {
    HIP_TRY(hipMemcpyAsync(st->dev, st->host, bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipEventRecord(st->ev, stream));
    st->busy = true;
    return BF_OK;
}
// the slot only lends its pinned buffer: copies to other device addresses were enqueued by the caller
bf_status stage_release_after(bf_scene::Stage *st, hipStream_t stream) {
    HIP_TRY(hipEventRecord(st->ev, stream));
    st->busy = true;
    return BF_OK;
}

static_assert(bf::kTopNodes == bfd::kTopNodes, "the builder's breadth-first prefix is what wf_trace caches");
static_assert(bfd::CTR_GUARD + 2 == bfd::CTR_COUNT && bfd::CTR_SURV_GUARD + 1 == bfd::CTR_COUNT,
              "the two sticky guard words are the last counters: renders clear the ones before them");

namespace {
struct TriMeta {
    uint32_t prim, shape;
    const float *n0, *n1, *n2;
    const float *uv0, *uv1, *uv2;
};
}  // namespace

// The triangle half of a description (endpoints_flatten has accepted its shapes): every mesh triangle for the BVH builder, in
// description order, and what its record carries besides the corners.
static bf_status gather_triangles(const bf_scene_desc *desc, std::vector<bf::BuildTri> &btris, std::vector<TriMeta> &meta, bool &any_normals,
                                  bool &any_uvs) {
    any_normals = any_uvs = false;
    uint32_t prim = 0;
    for (uint32_t i = 0; i < desc->n_shapes; ++i) {
        const bf_shape &s = desc->shapes[i];
        if (s.type != BF_SHAPE_MESH) {
            prim += 1;      // a rectangle
            continue;
        }
        for (uint32_t f = 0; f < s.n_faces; ++f) {
            uint32_t i0 = s.indices[3 * f], i1 = s.indices[3 * f + 1], i2 = s.indices[3 * f + 2];
            if (i0 >= s.n_vertices || i1 >= s.n_vertices || i2 >= s.n_vertices)
                return fail(BF_ERR_INVALID, "shape %u face %u: vertex index out of range", i, f);
            bf::BuildTri t;
            std::memcpy(t.p0, s.positions + 3 * i0, 12);
            std::memcpy(t.p1, s.positions + 3 * i1, 12);
            std::memcpy(t.p2, s.positions + 3 * i2, 12);
            btris.push_back(t);
            TriMeta m{prim + f, i, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
            if (s.texcoords) {
                m.uv0 = s.texcoords + 2 * i0;
                m.uv1 = s.texcoords + 2 * i1;
                m.uv2 = s.texcoords + 2 * i2;
                any_uvs = true;
            }
            if (s.normals) {
                m.n0 = s.normals + 3 * i0;
                m.n1 = s.normals + 3 * i1;
                m.n2 = s.normals + 3 * i2;
                any_normals = true;
            }
            meta.push_back(m);
        }
        prim += s.n_faces;
    }
    return BF_OK;
}

bf_status bf_scene_create(const bf_scene_desc *desc, bf_scene **out) {
    if (!desc || !out) return fail(BF_ERR_INVALID, "null argument");
    *out = nullptr;
    EndpointState::Image ends;
    std::vector<bf::BuildTri> btris;
    std::vector<TriMeta> meta;
    bool any_normals = false, any_uvs = false;
    {
        bf_status fst = endpoints_flatten(desc, ends);
        if (fst == BF_OK) fst = gather_triangles(desc, btris, meta, any_normals, any_uvs);
        if (fst != BF_OK) return fst;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(BF_ERR_DEVICE, "no HIP device available: the HIP path has no CPU fallback");
    const float origin_scale = ends.origin_scale;

    bf_scene *sc = new (std::nothrow) bf_scene();
    if (!sc) return fail(BF_ERR_NOMEM, "out of host memory");
    std::memset(&sc->d, 0, sizeof(sc->d));
    std::memset(&sc->info, 0, sizeof(sc->info));
    sc->tun = read_tunables();
    sc->geom = std::make_shared<bf_geometry>();
    sc->geom_token = std::make_shared<char>(0);
    sc->peers_rolling = std::make_shared<std::atomic<int>>(0);
    sc->mesh.origin_scale_built = origin_scale;
    // what a vertex update needs of the description later (bf_scene_update_vertices): every mesh's sizes, first primitive and indices
    sc->geom->topo.resize(desc->n_shapes);
    for (uint32_t i = 0; i < desc->n_shapes; ++i) {
        const bf_shape &s = desc->shapes[i];
        if (s.type != BF_SHAPE_MESH || !s.n_faces) continue;
        bf_geometry::MeshTopo &tp = sc->geom->topo[i];
        tp.n_vertices = s.n_vertices;
        tp.n_faces = s.n_faces;
        tp.has_normals = s.normals != nullptr;
        tp.indices.assign(s.indices, s.indices + 3 * (size_t) s.n_faces);
    }
    for (size_t t = meta.size(); t-- > 0;) sc->geom->topo[meta[t].shape].prim0 = meta[t].prim;      // (faces in order: the first one's)
    bf::BVH bvh;
    bf::build_bvh(btris, bvh, origin_scale);
    bf::BVH4 bvh4;
    bf::collapse_bvh4(bvh, bvh4);
    // sixteen-wide collapse of the same tree for the tail kernel's row traversal (bf_bvh.h: Node16)
    bf::BVH16 bvh16;
    bf::collapse_bvh16(bvh, bvh16);
    // a gang of R rows pops R entries per step: its stack holds at most one block of 16 R children per tree level
    // (blocks are consumed last-in first-out and a block's shallowest entry lies deeper than the block below it)
    uint32_t wide_rlog = 2;
    while (wide_rlog > 0 && (16u << wide_rlog) * std::max(1u, bvh16.max_depth) > (uint32_t) bfd::kWideStack) --wide_rlog;
    const bool use_wide = !btris.empty() && 16u * std::max(1u, bvh16.max_depth) <= (uint32_t) bfd::kWideStack &&
                          btris.size() < (1u << 27) && !sc->tun.no_wide;
    if (sc->tun.wide_rows_log >= 0) wide_rlog = std::min<uint32_t>(wide_rlog, (uint32_t) sc->tun.wide_rows_log);
    // ray origins also lie on the meshes: the largest |coordinate| of a vertex (the vertices themselves, as bf_scene_rebuild_bvh
    // takes them: the builder's padded scene box would overstate the bound by its own padding)
    for (const bf::BuildTri &t : btris)
        for (int k = 0; k < 3; ++k)
            sc->mesh.origin_scale_built = std::max({sc->mesh.origin_scale_built, std::fabs(t.p0[k]), std::fabs(t.p1[k]), std::fabs(t.p2[k])});
    // (+ kTriPad rows of padding behind the last triangle)
    std::vector<float4> tri_data(bfd::kTriStride * btris.size() + (btris.empty() ? 0 : kTriPad), make_float4(0, 0, 0, 0)), nrm_data;
    if (any_normals) nrm_data.resize(3 * btris.size());
    std::vector<float4> uv_data;
    if (any_uvs) uv_data.assign(3 * btris.size(), make_float4(0, 0, 0, 0));      // differences | (uv0, uv1) | (uv2, -, -): bf_device.h
    for (size_t slot = 0; slot < btris.size(); ++slot) {
        uint32_t src = bvh.order[slot];
        const bf::BuildTri &t = btris[src];
        const TriMeta &m = meta[src];
        if (desc->n_materials > 0xfffu || desc->n_emitters > 0xffeu) {
            bf_scene_destroy(sc);
            return fail(BF_ERR_UNSUPPORTED, "more than 4095 materials or 4094 emitters");
        }
        // tag word: bit 0 = has vertex normals, bit 1 = has texture coordinates, bits 8..19 = material,
        // bits 20..31 = emitter + 1 (bf_device_core.h)
        const bf_shape &msh = desc->shapes[m.shape];
        uint32_t has_n = (m.n0 ? 1u : 0u) | (m.uv0 ? 2u : 0u) | ((uint32_t) msh.material << 8) | ((uint32_t) (msh.emitter + 1) << 20);
        if (m.uv0)   // mesh.cpp:494-499: duv0 = uv1 - uv0, duv1 = uv2 - uv0
        {
            uv_data[slot] = make_float4(m.uv1[0] - m.uv0[0], m.uv1[1] - m.uv0[1], m.uv2[0] - m.uv0[0], m.uv2[1] - m.uv0[1]);
            uv_data[btris.size() + slot] = make_float4(m.uv0[0], m.uv0[1], m.uv1[0], m.uv1[1]);
            uv_data[2 * btris.size() + slot] = make_float4(m.uv2[0], m.uv2[1], 0.f, 0.f);
        }
        float w0, w1, w2;
        std::memcpy(&w0, &m.prim, 4);
        std::memcpy(&w1, &m.shape, 4);
        std::memcpy(&w2, &has_n, 4);
        tri_data[bfd::kTriStride * slot + 0] = make_float4(t.p0[0], t.p0[1], t.p0[2], w0);
        tri_data[bfd::kTriStride * slot + 1] = make_float4(t.p1[0], t.p1[1], t.p1[2], w1);
        tri_data[bfd::kTriStride * slot + 2] = make_float4(t.p2[0], t.p2[1], t.p2[2], w2);
        if (any_normals) {
            if (m.n0) {
                nrm_data[3 * slot + 0] = make_float4(m.n0[0], m.n0[1], m.n0[2], 0.f);
                nrm_data[3 * slot + 1] = make_float4(m.n1[0], m.n1[1], m.n1[2], 0.f);
                nrm_data[3 * slot + 2] = make_float4(m.n2[0], m.n2[1], m.n2[2], 0.f);
            } else {
                nrm_data[3 * slot + 0] = nrm_data[3 * slot + 1] = nrm_data[3 * slot + 2] = make_float4(0, 0, 0, 0);
            }
        }
    }
    std::vector<float4> node_data(8 * bvh4.nodes.size());
    if (!bvh4.nodes.empty()) std::memcpy(node_data.data(), bvh4.nodes.data(), bvh4.nodes.size() * sizeof(bf::Node4));
    // 64-byte quantised copy of the four-wide nodes for wf_trace (bf_bvh.h: Node4Q).  OPT-IN (BF_QUANT_BVH=1): four loads
    // per node step instead of seven, but +39 VALU operations and 1.3 % more node visits — measured 3 % SLOWER on C2
    // (wf_trace 4.33 -> 4.45 ms per step; the kernel waits on dependent fetches and on its half-busy VALU, not on the
    // number of vector-memory instructions: DESIGN.md 3.1), so the fp32 nodes stay the default.
    std::vector<float4> qnode_data;
    if (!bvh4.nodes.empty() && sc->tun.quant) {
        std::vector<bf::Node4Q> q;
        bf::quantise_bvh4(bvh4, q);
        qnode_data.resize(4 * q.size());
        std::memcpy(qnode_data.data(), q.data(), q.size() * sizeof(bf::Node4Q));
    }
    std::vector<float4> wnode_data;
    if (use_wide) {
        // one spare node of padding: a row's speculative third load of a child record may touch the next 16 bytes
        wnode_data.assign(32 * (bvh16.nodes.size() + 1), make_float4(0, 0, 0, 0));
        if (!bvh16.nodes.empty()) std::memcpy(wnode_data.data(), bvh16.nodes.data(), bvh16.nodes.size() * sizeof(bf::Node16));
    }
    (void) hipGetDevice(&sc->device);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, sc->device) == hipSuccess) sc->n_cus = prop.multiProcessorCount;

    uint64_t bytes = 0;
    bf_status st;
    // traversal-stack overflow columns: kernels keep >= 16 entries in LDS and launch at most
    // n_cus * kTraceBlocksPerCU workgroups
    {
        const uint32_t stride = (uint32_t) sc->n_cus * bfd::kTraceBlocksPerCU * bfd::kBlock;
        const uint32_t depth = bvh4.stack_need > 16 ? bvh4.stack_need - 16 : 1;
        void *p = nullptr;
        hipError_t he = hipMalloc(&p, (size_t) stride * depth * sizeof(int));
        if (he != hipSuccess) {
            bf_scene_destroy(sc);
            return fail(BF_ERR_NOMEM, "hipMalloc(traversal spill, %zu bytes): %s", (size_t) stride * depth * sizeof(int), hipGetErrorString(he));
        }
        sc->owned.push_back(p);
        bytes += (uint64_t) stride * depth * sizeof(int);
        sc->d.spill = (int *) p;
        sc->d.spill_stride = stride;
        sc->d.stack_need = bvh4.stack_need;
    }
    std::vector<void *> &gown = sc->geom->owned;
    if ((st = upload(node_data, &sc->d.nodes, gown, bytes)) != BF_OK || (st = upload(qnode_data, &sc->d.qnodes, gown, bytes)) != BF_OK ||
        (st = upload(wnode_data, &sc->d.wnodes, gown, bytes)) != BF_OK || (st = upload(tri_data, &sc->d.tris, gown, bytes)) != BF_OK ||
        (st = upload(nrm_data, &sc->d.normals, gown, bytes)) != BF_OK || (st = upload(uv_data, &sc->d.uvs, gown, bytes)) != BF_OK ||
        (st = endpoints_create(sc, ends, &bytes)) != BF_OK) {      // (the endpoint tables and the profile: bf_endpoints.cpp)
        bf_scene_destroy(sc);
        return st;
    }
    sc->d.n_tris = (uint32_t) btris.size();
    sc->d.n_nodes = (uint32_t) bvh4.nodes.size();
    sc->d.root = bvh4.root_child;
    sc->d.wroot = use_wide ? bvh16.root_child : bfd_no_node();
    sc->d.n_wnodes = use_wide ? (uint32_t) bvh16.nodes.size() : 0u;
    sc->d.wrows_log = wide_rlog;

    hipError_t e = hipMalloc((void **) &sc->run.counters, sizeof(unsigned long long) * bfd::CTR_COUNT);
    if (e == hipSuccess) e = hipMemset(sc->run.counters, 0, sizeof(unsigned long long) * bfd::CTR_COUNT);
    if (e != hipSuccess) {
        bf_scene_destroy(sc);
        return fail(BF_ERR_DEVICE, "hipMalloc(counters): %s", hipGetErrorString(e));
    }

    bf_scene_info &inf = sc->info;
    inf.n_shapes = desc->n_shapes;
    inf.n_rects = sc->d.n_rects;
    inf.n_triangles = sc->d.n_tris;
    inf.n_bvh_nodes = sc->d.n_nodes;
    inf.node_bytes = (uint32_t) sizeof(bf::Node4);
    inf.trace_node_bytes = sc->d.qnodes ? (uint32_t) sizeof(bf::Node4Q) : (uint32_t) sizeof(bf::Node4);
    inf.tri_bytes = 16 * bfd::kTriStride;
    inf.bvh_depth = bvh4.max_depth;
    inf.bvh_stack_need = bvh4.stack_need;
    inf.device_bytes = bytes;
    for (int k = 0; k < 3; ++k) {
        inf.bbox_min[k] = bvh.lo[k];
        inf.bbox_max[k] = bvh.hi[k];
    }
    *out = sc;
    return BF_OK;
}

bf_status bf_scene_read_bvh(const bf_scene *scene, uint32_t width, void *nodes_out, uint64_t nodes_bytes, float *tri_rows_out, int32_t *root_child) {
    if (!scene) return fail(BF_ERR_INVALID, "bf_scene_read_bvh: null scene");
    if (width != 4u && width != 16u) return fail(BF_ERR_INVALID, "bf_scene_read_bvh: width %u (4 or 16)", width);
    BF_ENTER(scene);
    {
        bf_status cst = close_sequence(scene, scene->run.roll.stream);
        if (cst != BF_OK) return cst;
    }
    HIP_TRY(scene->run.last.wait());
    if (width == 16u && !scene->d.wnodes) return fail(BF_ERR_UNSUPPORTED, "bf_scene_read_bvh: the scene has no sixteen-wide tree");
    const uint64_t need = width == 4u ? (uint64_t) scene->d.n_nodes * sizeof(bf::Node4) : (uint64_t) scene->d.n_wnodes * sizeof(bf::Node16);
    if (nodes_bytes < need || (need && !nodes_out))
        return fail(BF_ERR_INVALID, "bf_scene_read_bvh: nodes_out needs %llu bytes (%llu given)", (unsigned long long) need, (unsigned long long) nodes_bytes);
    if (need) HIP_TRY(hipMemcpy(nodes_out, width == 4u ? scene->d.nodes : scene->d.wnodes, need, hipMemcpyDeviceToHost));
    if (tri_rows_out && scene->d.n_tris)
        HIP_TRY(hipMemcpy(tri_rows_out, scene->d.tris, (size_t) scene->d.n_tris * bfd::kTriStride * sizeof(float4), hipMemcpyDeviceToHost));
    if (root_child) *root_child = width == 4u ? scene->d.root : scene->d.wroot;
    return BF_OK;
}

bf_status bf_scene_get_info(const bf_scene *scene, bf_scene_info *info) {
    if (!scene || !info) return fail(BF_ERR_INVALID, "null argument");
    *info = scene->info;
    info->device = scene->device;
    return BF_OK;
}

bf_status bf_scene_clone(const bf_scene *src, bf_scene **out) {
    if (!src || !out) return fail(BF_ERR_INVALID, "null argument");
    *out = nullptr;
    BF_ENTER(src);
    {
        bf_status cst = close_sequence(src, src->run.roll.stream);
        if (cst != BF_OK) return cst;
    }
    HIP_TRY(hipDeviceSynchronize());      // pending endpoint updates / translations of `src` are part of what is cloned
    bf_scene *sc = new (std::nothrow) bf_scene();
    if (!sc) return fail(BF_ERR_NOMEM, "out of host memory");
    sc->d = src->d;                        // geometry pointers shared (as they stand now); the rest replaced below
    sc->tun = src->tun;
    sc->geom = src->geom;
    sc->geom_token = src->geom_token;      // replaced below if the clone takes its own snapshot
    sc->peers_rolling = src->peers_rolling;
    sc->info = src->info;
    sc->device = src->device;
    sc->n_cus = src->n_cus;
    sc->run.aov.n = src->run.aov.n;        // the AOV table (bf_scene_set_aovs); the side rows are each handle's own
    std::memcpy(sc->run.aov.types, src->run.aov.types, sizeof(sc->run.aov.types));
    bf_status st = BF_OK;
    auto fail_out = [&](bf_status s) {
        bf_scene_destroy(sc);
        return s;
    };
    // own small tables (endpoints may differ per clone), own spill columns and counters
    if ((st = mesh_clone_snapshot(src, sc)) != BF_OK) return fail_out(st);      // the padding bound; the geometry `src` renders now, if it has moved
    if ((st = endpoints_clone(src, sc)) != BF_OK) return fail_out(st);
    {
        const uint32_t depth = src->d.stack_need > 16 ? src->d.stack_need - 16 : 1;
        void *p = nullptr;
        hipError_t e = hipMalloc(&p, (size_t) src->d.spill_stride * depth * sizeof(int));
        if (e != hipSuccess) return fail_out(fail(BF_ERR_NOMEM, "bf_scene_clone: traversal spill: %s", hipGetErrorString(e)));
        sc->owned.push_back(p);
        sc->d.spill = (int *) p;
    }
    {
        hipError_t e = hipMalloc((void **) &sc->run.counters, sizeof(unsigned long long) * bfd::CTR_COUNT);
        if (e == hipSuccess) e = hipMemset(sc->run.counters, 0, sizeof(unsigned long long) * bfd::CTR_COUNT);
        if (e != hipSuccess) return fail_out(fail(BF_ERR_DEVICE, "bf_scene_clone: counters: %s", hipGetErrorString(e)));
    }
    *out = sc;
    return BF_OK;
}


/* developer probe (tools/fetch_probe.py): `reps` launches of the gather pattern `mode` over a table of 2^log2_rows 16-byte rows
   (a second buffer of the same size is streamed in between, so every launch starts with a cold L2); returns the mean ms */
bf_status bfdbg_gather_probe(int mode, uint32_t log2_rows, uint32_t reps, float *ms_out) {
    if (mode < 0 || mode > 2 || log2_rows < 10 || log2_rows > 28 || reps == 0) return fail(BF_ERR_INVALID, "bfdbg_gather_probe: bad arguments");
    const uint32_t n = 1u << log2_rows;
    float4 *table = nullptr, *flush = nullptr, *out = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipMalloc((void **) &table, (size_t) n * 16);
    if (e == hipSuccess) e = hipMalloc((void **) &flush, (size_t) n * 16);
    if (e == hipSuccess) e = hipMalloc((void **) &out, 1024 * 16);
    if (e == hipSuccess) e = hipMemset(table, 0, (size_t) n * 16);
    if (e == hipSuccess) e = hipMemset(flush, 0, (size_t) n * 16);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    float total = 0.f;
    for (uint32_t r = 0; r < reps && e == hipSuccess; ++r) {
        e = hipMemsetAsync(flush, (int) (r & 1u), (size_t) n * 16, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e0, nullptr);
        if (e == hipSuccess) e = bfk_gather_probe(mode, table, n, out, nullptr);
        if (e == hipSuccess) e = hipEventRecord(e1, nullptr);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        total += ms;
    }
    if (e0) (void) hipEventDestroy(e0);
    if (e1) (void) hipEventDestroy(e1);
    (void) hipFree(table);
    (void) hipFree(flush);
    (void) hipFree(out);
    if (e != hipSuccess) return fail(BF_ERR_DEVICE, "bfdbg_gather_probe: %s", hipGetErrorString(e));
    if (ms_out) *ms_out = total / (float) reps;
    return BF_OK;
}

/* test hook: take (1) / release (0) the handle's busy flag, as a call of another host thread would hold it */
bf_status bfdbg_hold_busy(bf_scene *scene, int on) {
    if (!scene) return fail(BF_ERR_INVALID, "null argument");
    if (on) {
        if (scene->busy.test_and_set(std::memory_order_acquire)) return fail(BF_ERR_INVALID, "bfdbg_hold_busy: already held");
    } else {
        scene->busy.clear(std::memory_order_release);
    }
    return BF_OK;
}


// ---------------------------------------------------------------------------
// One process, several GPUs (bf_launch.device_mask; 8e: sample shards + one all-reduce).  Paths are i.i.d.:
// GPU g of G renders the global path indices bf_shard_range(n, g, G) of the launch through bf_launch.path_offset — the
// union is the sample set of a one-GPU render — and the per-GPU range histograms are summed by ONE ncclAllReduce(float,
// sum) over xGMI.  RCCL is loaded on first use (dlopen: a process that never shards needs no librccl, and one that
// already carries a copy — PyTorch ships its own — keeps using that one).
// ---------------------------------------------------------------------------
void bf_shard_range(uint64_t n_paths, uint32_t shard, uint32_t n_shards, uint64_t *offset, uint64_t *count) {
    if (n_shards == 0) n_shards = 1;
    // floor(n s / S) without overflowing 64 bits for n < 2^63, S < 2^32
    auto cut = [&](uint64_t k) -> uint64_t { return (uint64_t) (((unsigned __int128) n_paths * k) / n_shards); };
    const uint64_t lo = cut(shard), hi = cut((uint64_t) shard + 1u);
    if (offset) *offset = lo;
    if (count) *count = hi - lo;
}

}  // extern "C"
namespace {
struct Rccl {
    void *lib = nullptr;
    decltype(&ncclCommInitAll) comm_init_all = nullptr;
    decltype(&ncclCommDestroy) comm_destroy = nullptr;
    decltype(&ncclAllReduce) all_reduce = nullptr;
    decltype(&ncclGroupStart) group_start = nullptr;
    decltype(&ncclGroupEnd) group_end = nullptr;
    decltype(&ncclGetErrorString) error_string = nullptr;
    std::string why;
};
Rccl &rccl() {
    static Rccl r = [] {
        Rccl q;
        // BF_RCCL_LIB names the library to load instead (a site build; the tests force the not-found path with it)
        const char *forced = getenv("BF_RCCL_LIB");
        const char *names[] = {forced && *forced ? forced : "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        const size_t n_names = forced && *forced ? 1 : 3;
        for (size_t i = 0; i < n_names && !q.lib; ++i)      // a copy that is already in the process (torch's) first
            q.lib = dlopen(names[i], RTLD_NOW | RTLD_NOLOAD | RTLD_LOCAL);
        std::string last;
        for (size_t i = 0; i < n_names && !q.lib; ++i) {
            q.lib = dlopen(names[i], RTLD_NOW | RTLD_LOCAL);
            if (!q.lib) {
                const char *e = dlerror();      // ONE call: dlerror() clears the message it returns
                last = e ? e : "";
            }
        }
        if (!q.lib) {
            q.why = std::string(forced && *forced ? forced : "librccl.so") + " not found: " + last;
            return q;
        }
        q.comm_init_all = (decltype(q.comm_init_all)) dlsym(q.lib, "ncclCommInitAll");
        q.comm_destroy = (decltype(q.comm_destroy)) dlsym(q.lib, "ncclCommDestroy");
        q.all_reduce = (decltype(q.all_reduce)) dlsym(q.lib, "ncclAllReduce");
        q.group_start = (decltype(q.group_start)) dlsym(q.lib, "ncclGroupStart");
        q.group_end = (decltype(q.group_end)) dlsym(q.lib, "ncclGroupEnd");
        q.error_string = (decltype(q.error_string)) dlsym(q.lib, "ncclGetErrorString");
        if (!q.comm_init_all || !q.comm_destroy || !q.all_reduce || !q.group_start || !q.group_end || !q.error_string) {
            q.why = "librccl.so lacks ncclCommInitAll / ncclAllReduce / ncclGroupStart / ncclGroupEnd";
            q.lib = nullptr;
        }
        return q;
    }();
    return r;
}
// one communicator set per ordered device list, created on first use and kept for the life of the process
std::mutex g_comm_mutex;
std::map<std::vector<int>, std::vector<ncclComm_t>> g_comms;
}  // namespace
extern "C" {

bf_status bf_allreduce_device(const int *devices, uint32_t n_devices, float *const *bufs, uint64_t count, void *const *streams) {
    if (!devices || !bufs || n_devices == 0) return fail(BF_ERR_INVALID, "bf_allreduce_device: null argument");
    if (count == 0) return BF_OK;
    for (uint32_t g = 0; g < n_devices; ++g)
        if (!bufs[g]) return fail(BF_ERR_INVALID, "bf_allreduce_device: buffer %u is null", g);
    Rccl &r = rccl();
    if (!r.lib) return fail(BF_ERR_UNSUPPORTED, "bf_allreduce_device: %s", r.why.c_str());
    std::vector<int> key(devices, devices + n_devices);
    for (uint32_t a = 0; a < n_devices; ++a)
        for (uint32_t b = a + 1; b < n_devices; ++b)
            if (key[a] == key[b]) return fail(BF_ERR_INVALID, "bf_allreduce_device: device %d is listed twice", key[a]);
    std::lock_guard<std::mutex> lock(g_comm_mutex);
    auto it = g_comms.find(key);
    if (it == g_comms.end()) {
        std::vector<ncclComm_t> comms(n_devices);
        ncclResult_t nr = r.comm_init_all(comms.data(), (int) n_devices, key.data());
        if (nr != ncclSuccess) return fail(BF_ERR_DEVICE, "ncclCommInitAll(%u devices): %s", n_devices, r.error_string(nr));
        it = g_comms.emplace(key, std::move(comms)).first;
    }
    int prev = -1;
    (void) hipGetDevice(&prev);
    ncclResult_t nr = r.group_start();
    for (uint32_t g = 0; g < n_devices && nr == ncclSuccess; ++g) {
        if (hipSetDevice(key[g]) != hipSuccess) {
            (void) r.group_end();
            if (prev >= 0) (void) hipSetDevice(prev);
            return fail(BF_ERR_DEVICE, "bf_allreduce_device: hipSetDevice(%d) failed", key[g]);
        }
        nr = r.all_reduce(bufs[g], bufs[g], (size_t) count, ncclFloat, ncclSum, it->second[g],
                          reinterpret_cast<hipStream_t>(streams ? streams[g] : nullptr));
    }
    ncclResult_t ne = r.group_end();
    if (prev >= 0) (void) hipSetDevice(prev);
    if (nr == ncclSuccess) nr = ne;
    if (nr != ncclSuccess) return fail(BF_ERR_DEVICE, "ncclAllReduce: %s", r.error_string(nr));
    return BF_OK;
}

bf_status bf_render_sharded_device(bf_scene *const *scenes, uint32_t n_devices, const bf_launch *launch, float *const *hist_dev,
                                   void *const *streams, bf_stats *stats_out) {
    if (!scenes || !launch || !hist_dev || n_devices == 0) return fail(BF_ERR_INVALID, "bf_render_sharded_device: null argument");
    if (launch->flags & BF_FLAG_EXACT_SUM)
        return fail(BF_ERR_UNSUPPORTED, "bf_render_sharded_device: BF_FLAG_EXACT_SUM is not supported (an all-reduce of floats would round once per shard; "
                                        "reducing the limbs across devices is a follow-up)");
    if (launch->flags & BF_FLAG_AOV)
        return fail(BF_ERR_UNSUPPORTED, "bf_render_sharded_device: BF_FLAG_AOV is not supported (the shards' handles each carry an AOV table "
                                        "of their own; render the AOVs per device)");
    if (launch->flags & BF_FLAG_CLASSES)
        return fail(BF_ERR_UNSUPPORTED, "bf_render_sharded_device: BF_FLAG_CLASSES is not supported (the shards' handles each carry a class table "
                                        "of their own; render the classes per device)");
    std::vector<int> devices(n_devices);
    for (uint32_t g = 0; g < n_devices; ++g) {
        if (!scenes[g] || !hist_dev[g]) return fail(BF_ERR_INVALID, "bf_render_sharded_device: scene / histogram %u is null", g);
        devices[g] = scenes[g]->device;
    }
    if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
    const bool rolling = (launch->flags & BF_FLAG_ROLLING) != 0u;
    if (stats_out && rolling)
        return fail(BF_ERR_INVALID, "BF_FLAG_ROLLING: a rolling render has no statistics of its own (bf_scene_flush reports the sequence's)");
    // Every GPU's launches are enqueued before any of them is waited for — also when statistics are asked for: a render
    // with stats_out is synchronous per device (it would make the GPUs take turns), so the shards are issued WITHOUT, each
    // between two events on its own stream, and the counters are read per device once all of them are in flight.
    std::vector<hipEvent_t> ev(stats_out ? 2 * (size_t) n_devices : 0, nullptr);
    std::vector<uint64_t> shard_paths(n_devices, 0);
    auto drop_events = [&]() {
        for (hipEvent_t e : ev)
            if (e) (void) hipEventDestroy(e);
    };
    for (uint32_t g = 0; g < n_devices; ++g) {
        bf_launch lg = *launch;
        uint64_t off = 0, cnt = 0;
        bf_shard_range(launch->n_paths, g, n_devices, &off, &cnt);
        lg.n_paths = cnt;
        lg.path_offset = launch->path_offset + off;
        shard_paths[g] = cnt;
        if (cnt == 0) continue;
        hipStream_t sg = reinterpret_cast<hipStream_t>(streams ? streams[g] : nullptr);
        if (stats_out) {
            DeviceGuard on_device(devices[g]);
            hipError_t he = hipEventCreate(&ev[2 * g]);
            if (he == hipSuccess) he = hipEventCreate(&ev[2 * g + 1]);
            if (he == hipSuccess) he = hipEventRecord(ev[2 * g], sg);
            if (he != hipSuccess) {
                drop_events();
                return fail(BF_ERR_DEVICE, "bf_render_sharded_device: device %d: %s", devices[g], hipGetErrorString(he));
            }
        }
        if (stats_out) lg.flags |= BF_FLAG_COUNT;      // (the counters are read below, once every device is in flight)
        bf_status st = bf_render_device(scenes[g], &lg, hist_dev[g], nullptr, sg, nullptr);
        if (st == BF_OK && stats_out) {
            DeviceGuard on_device(devices[g]);
            if (hipEventRecord(ev[2 * g + 1], sg) != hipSuccess) st = fail(BF_ERR_DEVICE, "bf_render_sharded_device: hipEventRecord failed");
        }
        if (st != BF_OK) {
            drop_events();
            return st;
        }
    }
    bf_status rst = BF_OK;
    // a rolling render's histogram is complete only after bf_scene_flush: the caller reduces then (bf_allreduce_device);
    // a communicator of one: the sum is the histogram itself
    if (!rolling && n_devices > 1) rst = bf_allreduce_device(devices.data(), n_devices, hist_dev, bf_launch_channels(launch), streams);
    if (stats_out) {
        unsigned long long lost = 0, refused = 0;
        for (uint32_t g = 0; g < n_devices && rst == BF_OK; ++g) {
            if (shard_paths[g] == 0) continue;
            BF_ENTER(scenes[g]);                 // (this handle's device; the counters are the handle's)
            hipError_t he = hipEventSynchronize(ev[2 * g + 1]);
            unsigned long long c[bfd::CTR_COUNT];
            if (he == hipSuccess) he = hipMemcpy(c, scenes[g]->run.counters, sizeof(c), hipMemcpyDeviceToHost);
            float ms = 0.f;
            if (he == hipSuccess) he = hipEventElapsedTime(&ms, ev[2 * g], ev[2 * g + 1]);
            if (he != hipSuccess) {
                rst = fail(BF_ERR_DEVICE, "bf_render_sharded_device: device %d: %s", devices[g], hipGetErrorString(he));
                break;
            }
            bf_stats p;
            fill_stats(scenes[g], c, shard_paths[g], &p);
            stats_out->n_paths += p.n_paths;
            stats_out->n_rays_closest += p.n_rays_closest;
            stats_out->n_rays_shadow += p.n_rays_shadow;
            stats_out->n_nodes_visited += p.n_nodes_visited;
            stats_out->n_tris_tested += p.n_tris_tested;
            stats_out->n_invalid += p.n_invalid;
            stats_out->n_bounces += p.n_bounces;
            stats_out->n_rays_tail += p.n_rays_tail;
            stats_out->n_rays_traced += p.n_rays_traced;
            stats_out->n_nodes_lds += p.n_nodes_lds;
            stats_out->kernel_variant = p.kernel_variant;
            // the devices run side by side: the slowest one's span (the per-kernel times need a synchronous render: 0 here)
            stats_out->kernel_ms = std::max(stats_out->kernel_ms, ms);
            if (c[bfd::CTR_GUARD] || c[bfd::CTR_SURV_GUARD]) {      // cleared per handle, reported once for all of them below
                lost += c[bfd::CTR_GUARD];
                refused += c[bfd::CTR_SURV_GUARD];
                (void) report_guards(scenes[g], c[bfd::CTR_GUARD], c[bfd::CTR_SURV_GUARD]);
            }
        }
        drop_events();
        if (rst == BF_OK && (lost || refused)) rst = guard_error(lost, refused);
    }
    return rst;
}

bf_status bf_render_sharded(bf_scene *const *scenes, uint32_t n_devices, const bf_launch *launch, float *hist_out, bf_stats *stats_out) {
    if (!scenes || !launch || !hist_out || n_devices == 0) return fail(BF_ERR_INVALID, "bf_render_sharded: null argument");
    if (launch->flags & BF_FLAG_EXACT_SUM)
        return fail(BF_ERR_UNSUPPORTED, "bf_render_sharded: BF_FLAG_EXACT_SUM is not supported (an all-reduce of floats would round once per shard; "
                                        "reducing the limbs across devices is a follow-up)");
    if (launch->flags & BF_FLAG_AOV)
        return fail(BF_ERR_UNSUPPORTED, "bf_render_sharded: BF_FLAG_AOV is not supported (the shards' handles each carry an AOV table of "
                                        "their own; render the AOVs per device)");
    if (launch->flags & BF_FLAG_CLASSES)
        return fail(BF_ERR_UNSUPPORTED, "bf_render_sharded: BF_FLAG_CLASSES is not supported (the shards' handles each carry a class table of "
                                        "their own; render the classes per device)");
    if (launch->flags & BF_FLAG_ROLLING) return fail(BF_ERR_INVALID, "bf_render_sharded: host-buffer renders are synchronous (no BF_FLAG_ROLLING)");
    const uint64_t n = bf_launch_channels(launch);
    if (n == 0) return fail(BF_ERR_INVALID, "unknown mode");
    int prev = -1;
    (void) hipGetDevice(&prev);
    std::vector<float *> bufs(n_devices, nullptr);
    auto cleanup = [&]() {
        for (uint32_t g = 0; g < n_devices; ++g)
            if (bufs[g] && scenes[g] && hipSetDevice(scenes[g]->device) == hipSuccess) (void) hipFree(bufs[g]);
        if (prev >= 0) (void) hipSetDevice(prev);
    };
    for (uint32_t g = 0; g < n_devices; ++g) {
        if (!scenes[g]) {
            cleanup();
            return fail(BF_ERR_INVALID, "bf_render_sharded: scene %u is null", g);
        }
        hipError_t e = hipSetDevice(scenes[g]->device);
        if (e == hipSuccess) e = hipMalloc((void **) &bufs[g], n * sizeof(float));
        if (e == hipSuccess) e = hipMemset(bufs[g], 0, n * sizeof(float));
        if (e != hipSuccess) {
            cleanup();
            return fail(BF_ERR_DEVICE, "bf_render_sharded: device %d: %s", scenes[g]->device, hipGetErrorString(e));
        }
    }
    bf_status st = bf_render_sharded_device(scenes, n_devices, launch, bufs.data(), nullptr, stats_out);
    for (uint32_t g = 0; g < n_devices && st == BF_OK; ++g) {
        hipError_t e = hipSetDevice(scenes[g]->device);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) st = fail(BF_ERR_DEVICE, "bf_render_sharded: device %d: %s", scenes[g]->device, hipGetErrorString(e));
    }
    if (st == BF_OK) {
        hipError_t e = hipSetDevice(scenes[0]->device);
        if (e == hipSuccess) e = hipMemcpy(hist_out, bufs[0], n * sizeof(float), hipMemcpyDeviceToHost);
        if (e != hipSuccess) st = fail(BF_ERR_DEVICE, "bf_render_sharded copy back: %s", hipGetErrorString(e));
    }
    cleanup();
    return st;
}

}  // extern "C"
// host buffers around a device render: `run(d_hist, d_rec, stats)` renders n_renders renders of `launch` into them
template <class Run>
static bf_status render_host_with(const bf_scene *scene, const bf_launch *launch, uint64_t n_renders, float *hist_out,
                                  bf_path_record *records_out, bf_stats *stats_out, Run &&run) {
    if (!scene || !launch || !hist_out) return fail(BF_ERR_INVALID, "null argument");
    if (n_renders == 0) return fail(BF_ERR_INVALID, "bf_render_batch: n_renders is 0");
    const uint64_t nchan = (uint64_t) bf_scene_launch_channels(scene, launch) * n_renders, n_rec = launch->n_paths * n_renders;
    if (nchan == 0) return fail(BF_ERR_INVALID, "unknown mode");
    DeviceGuard on_device(scene->device);      // the staging buffers live where the kernels run, whatever the caller's current device
    float *d_hist = nullptr;
    bf_path_record *d_rec = nullptr;
    HIP_TRY(hipMalloc((void **) &d_hist, nchan * sizeof(float)));
    hipError_t e = hipMemset(d_hist, 0, nchan * sizeof(float));
    if (e == hipSuccess && records_out && n_rec)
        e = hipMalloc((void **) &d_rec, n_rec * sizeof(bf_path_record));
    if (e != hipSuccess) {
        (void) hipFree(d_hist);
        return fail(BF_ERR_DEVICE, "bf_render: %s", hipGetErrorString(e));
    }
    bf_stats local;
    bf_status st = run(d_hist, d_rec, stats_out ? stats_out : &local);
    if (st == BF_OK) {
        e = hipMemcpy(hist_out, d_hist, nchan * sizeof(float), hipMemcpyDeviceToHost);
        if (e == hipSuccess && d_rec)
            e = hipMemcpy(records_out, d_rec, n_rec * sizeof(bf_path_record), hipMemcpyDeviceToHost);
        if (e != hipSuccess) st = fail(BF_ERR_DEVICE, "bf_render copy back: %s", hipGetErrorString(e));
    }
    (void) hipFree(d_hist);
    if (d_rec) (void) hipFree(d_rec);
    return st;
}
extern "C" {

static bf_status render_host(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, float *hist_out,
                             bf_path_record *records_out, bf_stats *stats_out) {
    return render_host_with(scene, launch, batch ? batch->n_renders : 1u, hist_out, records_out, stats_out,
                            [&](float *h, bf_path_record *r, bf_stats *st) {
                                return batch ? bf_render_batch_device(scene, launch, batch, h, r, nullptr, st) : bf_render_device(scene, launch, h, r, nullptr, st);
                            });
}

bf_status bf_render_motion_batch(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_shapes,
                                 const float *to_world, float *hist_out, bf_path_record *records_out, bf_stats *stats_out) {
    if (n_renders == 0) return fail(BF_ERR_INVALID, "bf_render_motion_batch: n_renders is 0");
    return render_host_with(scene, launch, n_renders, hist_out, records_out, stats_out, [&](float *h, bf_path_record *r, bf_stats *st) {
        return bf_render_motion_batch_device(scene, launch, n_renders, seeds, n_shapes, to_world, h, r, nullptr, st);
    });
}

bf_status bf_render_deform_batch(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_deform,
                                 const uint32_t *shapes, const float *const *positions, const float *const *normals, uint32_t n_shapes,
                                 const float *to_world, float *hist_out, bf_path_record *records_out, bf_stats *stats_out) {
    const char *fn = "bf_render_deform_batch:";
    if (!scene || (n_deform && (!shapes || !positions))) return fail(BF_ERR_INVALID, "%s null argument", fn);
    if (n_renders == 0) return fail(BF_ERR_INVALID, "%s n_renders is 0", fn);
    // the host arrays are checked here (finite; their largest |coordinate| is the bound the device form is given), the rest there
    std::vector<size_t> count(n_deform, 0);
    float bound = 0.f;
    for (uint32_t j = 0; j < n_deform; ++j) {
        const bf_geometry::MeshTopo *tp = nullptr;
        const float *nj = normals ? normals[j] : nullptr;
        bf_status cst = check_deform_shape(scene, shapes[j], nj != nullptr, fn, &tp);
        if (cst != BF_OK) return cst;
        if (!positions[j]) return fail(BF_ERR_INVALID, "%s shape %u: null positions", fn, shapes[j]);
        count[j] = (size_t) n_renders * 3 * tp->n_vertices;
        for (size_t i = 0; i < count[j]; ++i) {
            if (!std::isfinite(positions[j][i]) || (nj && !std::isfinite(nj[i])))
                return fail(BF_ERR_INVALID, "%s render %zu, shape %u: non-finite value at vertex %zu", fn, i / (3 * (size_t) tp->n_vertices), shapes[j],
                            (i / 3) % tp->n_vertices);
            bound = std::max(bound, std::fabs(positions[j][i]));
        }
    }
    bound = std::max(bound, std::numeric_limits<float>::min());
    DeviceGuard on_device(scene->device);
    std::vector<void *> tmp;
    std::vector<const float *> dpos(n_deform, nullptr), dnrm(n_deform, nullptr);
    auto cleanup = [&]() {
        for (void *p : tmp) (void) hipFree(p);
    };
    auto up = [&](const float *from, size_t n, const float **out) -> hipError_t {
        *out = nullptr;
        if (!from || !n) return hipSuccess;
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, n * sizeof(float));
        if (e != hipSuccess) return e;
        tmp.push_back(q);
        *out = (const float *) q;
        return hipMemcpy(q, from, n * sizeof(float), hipMemcpyHostToDevice);
    };
    for (uint32_t j = 0; j < n_deform; ++j) {
        hipError_t e = up(positions[j], count[j], &dpos[j]);
        if (e == hipSuccess && normals) e = up(normals[j], count[j], &dnrm[j]);
        if (e != hipSuccess) {
            cleanup();
            return fail(BF_ERR_NOMEM, "%s shape %u: %s", fn, shapes[j], hipGetErrorString(e));
        }
        if (!dpos[j]) dpos[j] = (const float *) (uintptr_t) 16;      // (a mesh without vertices: never read)
    }
    bf_status st = render_host_with(scene, launch, n_renders, hist_out, records_out, stats_out, [&](float *h, bf_path_record *r, bf_stats *s) {
        return bf_render_deform_batch_device(scene, launch, n_renders, seeds, n_deform, shapes, dpos.data(), normals ? dnrm.data() : nullptr, bound,
                                             n_shapes, to_world, h, r, nullptr, s);
    });
    (void) hipDeviceSynchronize();      // the renders read the arrays freed below
    cleanup();
    return st;
}

bf_status bf_render_skin_batch(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_skinned,
                               const uint32_t *shapes, const float *const *bones, uint32_t n_shapes, const float *to_world, float *hist_out,
                               bf_path_record *records_out, bf_stats *stats_out) {
    if (n_renders == 0) return fail(BF_ERR_INVALID, "bf_render_skin_batch: n_renders is 0");
    // the bone tables are host arrays in both forms: only the histogram and the records differ
    return render_host_with(scene, launch, n_renders, hist_out, records_out, stats_out, [&](float *h, bf_path_record *r, bf_stats *st) {
        return bf_render_skin_batch_device(scene, launch, n_renders, seeds, n_skinned, shapes, bones, n_shapes, to_world, h, r, nullptr, st);
    });
}

bf_status bf_render_morph_batch(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, uint32_t n_morphed,
                                const uint32_t *shapes, const float *const *weights, const float *const *bones, uint32_t n_shapes,
                                const float *to_world, float *hist_out, bf_path_record *records_out, bf_stats *stats_out) {
    if (n_renders == 0) return fail(BF_ERR_INVALID, "bf_render_morph_batch: n_renders is 0");
    // the weights and the bone tables are host arrays in both forms: only the histogram and the records differ
    return render_host_with(scene, launch, n_renders, hist_out, records_out, stats_out, [&](float *h, bf_path_record *r, bf_stats *st) {
        return bf_render_morph_batch_device(scene, launch, n_renders, seeds, n_morphed, shapes, weights, bones, n_shapes, to_world, h, r, nullptr, st);
    });
}

bf_status bf_render(const bf_scene *scene, const bf_launch *launch, float *hist_out, bf_path_record *records_out,
                    bf_stats *stats_out) {
    return render_host(scene, launch, nullptr, hist_out, records_out, stats_out);
}

bf_status bf_render_batch(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, float *hist_out,
                          bf_path_record *records_out, bf_stats *stats_out) {
    if (!batch) return fail(BF_ERR_INVALID, "bf_render_batch: null batch");
    return render_host(scene, launch, batch, hist_out, records_out, stats_out);
}

static bf_status trace_common(const bf_scene *scene, uint64_t n, const float *rays, int any_hit, float *out_t,
                              uint32_t *out_prim, uint32_t *out_shape, float *out_uv, uint8_t *out_hit,
                              float *out_si = nullptr) {
    if (!scene || (n && !rays)) return fail(BF_ERR_INVALID, "null argument");
    if (n == 0) return BF_OK;
    DeviceGuard on_device(scene->device);
    float *d_rays = nullptr, *d_t = nullptr, *d_uv = nullptr, *d_si = nullptr;
    uint32_t *d_prim = nullptr, *d_shape = nullptr;
    uint8_t *d_hit = nullptr;
    std::vector<void *> tmp;
    auto alloc = [&](void **p, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) tmp.push_back(*p);
        return e;
    };
    auto cleanup = [&]() {
        for (void *p : tmp) (void) hipFree(p);
    };
    hipError_t e = alloc((void **) &d_rays, n * 8 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_rays, rays, n * 8 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && any_hit) e = alloc((void **) &d_hit, n);
    if (e == hipSuccess && !any_hit) {
        e = alloc((void **) &d_t, n * 4);
        if (e == hipSuccess) e = alloc((void **) &d_prim, n * 4);
        if (e == hipSuccess) e = alloc((void **) &d_shape, n * 4);
        if (e == hipSuccess) e = alloc((void **) &d_uv, n * 8);
        if (e == hipSuccess && out_si) e = alloc((void **) &d_si, n * BF_SI_FLOATS * sizeof(float));
    }
    if (e == hipSuccess) e = bfk_launch_trace(&scene->d, n, d_rays, any_hit, d_t, d_prim, d_shape, d_uv, d_hit, d_si, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess && any_hit && out_hit) e = hipMemcpy(out_hit, d_hit, n, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !any_hit) {
        if (out_t) e = hipMemcpy(out_t, d_t, n * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && out_prim) e = hipMemcpy(out_prim, d_prim, n * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && out_shape) e = hipMemcpy(out_shape, d_shape, n * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess && out_uv) e = hipMemcpy(out_uv, d_uv, n * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess && out_si) e = hipMemcpy(out_si, d_si, n * BF_SI_FLOATS * sizeof(float), hipMemcpyDeviceToHost);
    }
    cleanup();
    if (e != hipSuccess) return fail(BF_ERR_DEVICE, "bf_trace: %s", hipGetErrorString(e));
    return BF_OK;
}

bf_status bf_trace_closest(const bf_scene *scene, uint64_t n, const float *rays, float *out_t, uint32_t *out_prim,
                           uint32_t *out_shape, float *out_uv) {
    return trace_common(scene, n, rays, 0, out_t, out_prim, out_shape, out_uv, nullptr);
}

bf_status bf_ray_intersect(const bf_scene *scene, uint64_t n, const float *rays, float *out_si, uint32_t *out_prim,
                           uint32_t *out_shape) {
    if (n && !out_si) return fail(BF_ERR_INVALID, "bf_ray_intersect: null output");
    return trace_common(scene, n, rays, 0, nullptr, out_prim, out_shape, nullptr, nullptr, out_si);
}

bf_status bf_trace_any(const bf_scene *scene, uint64_t n, const float *rays, uint8_t *out_hit) {
    return trace_common(scene, n, rays, 1, nullptr, nullptr, nullptr, nullptr, out_hit);
}

bf_status bf_eval_elementary(int op, uint64_t n, const float *x, float *y) {
    if (op < 0 || op > 6 || (n && (!x || !y))) return fail(BF_ERR_INVALID, "bf_eval_elementary: bad arguments");
    if (n == 0) return BF_OK;
    float *d_x = nullptr, *d_y = nullptr;
    hipError_t e = hipMalloc((void **) &d_x, n * 4);
    if (e == hipSuccess) e = hipMalloc((void **) &d_y, n * 4);
    if (e == hipSuccess) e = hipMemcpy(d_x, x, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = bfk_launch_elementary(op, n, d_x, d_y);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(y, d_y, n * 4, hipMemcpyDeviceToHost);
    (void) hipFree(d_x);
    (void) hipFree(d_y);
    if (e != hipSuccess) return fail(BF_ERR_DEVICE, "bf_eval_elementary: %s", hipGetErrorString(e));
    return BF_OK;
}

// ---- the exact accumulator on caller-given addends (include/beifong_hip.h; bf_sum.h) ----
static bf_status exact_sum_check(const char *fn, uint64_t n, const uint32_t *cell, const float *value, uint32_t n_cells, const float *out) {
    if (!out || !n_cells || (n && (!cell || !value))) return fail(BF_ERR_INVALID, "%s: null argument", fn);
    if (n >= bfs::kMaxAddends) return fail(BF_ERR_INVALID, "%s: n %llu is not below 2^31, the addends a cell is exact for", fn, (unsigned long long) n);
    for (uint64_t i = 0; i < n; ++i) {
        if (cell[i] >= n_cells) return fail(BF_ERR_INVALID, "%s: cell[%llu] = %u is not below n_cells %u", fn, (unsigned long long) i, cell[i], n_cells);
        if (!std::isfinite(value[i])) return fail(BF_ERR_INVALID, "%s: value[%llu] is not finite", fn, (unsigned long long) i);
    }
    return BF_OK;
}

bf_status bf_exact_sum_host(uint64_t n, const uint32_t *cell, const float *value, uint32_t n_cells, float *out) {
    bf_status st = exact_sum_check("bf_exact_sum_host", n, cell, value, n_cells, out);
    if (st != BF_OK) return st;
    std::vector<int64_t> limbs((size_t) n_cells * bfs::kLimbs, 0);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t bits;
        std::memcpy(&bits, &value[i], sizeof(bits));
        bfs::add(&limbs[(size_t) cell[i] * bfs::kLimbs], bits);
    }
    for (uint32_t c = 0; c < n_cells; ++c) {
        const uint32_t bits = bfs::resolve(&limbs[(size_t) c * bfs::kLimbs]).bits;
        std::memcpy(&out[c], &bits, sizeof(bits));
    }
    return BF_OK;
}

bf_status bf_exact_sum(uint64_t n, const uint32_t *cell, const float *value, uint32_t n_cells, uint32_t in_lds, float *out) {
    bf_status st = exact_sum_check("bf_exact_sum", n, cell, value, n_cells, out);
    if (st != BF_OK) return st;
    uint32_t *d_cell = nullptr;
    float *d_value = nullptr, *d_out = nullptr;
    void *d_limbs = nullptr;
    const size_t limb_bytes = (size_t) n_cells * bfs::kLimbs * sizeof(int64_t);
    // privatised like a render's histogram: when the cells fit what kMaxLdsHist stands for
    const bool lds = in_lds && (uint64_t) n_cells * bfs::kCellFloats <= (uint64_t) bfd::kMaxLdsHist;
    hipError_t e = hipMalloc(&d_limbs, limb_bytes);
    if (e == hipSuccess) e = hipMalloc((void **) &d_out, (size_t) n_cells * 4);
    if (e == hipSuccess && n) e = hipMalloc((void **) &d_cell, n * 4);
    if (e == hipSuccess && n) e = hipMalloc((void **) &d_value, n * 4);
    if (e == hipSuccess && n) e = hipMemcpy(d_cell, cell, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && n) e = hipMemcpy(d_value, value, n * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(d_limbs, 0, limb_bytes);
    if (e == hipSuccess) e = hipMemset(d_out, 0, (size_t) n_cells * 4);
    if (e == hipSuccess && n) {
        const unsigned grid = (unsigned) std::min<uint64_t>((n + bfd::kBlock - 1) / bfd::kBlock, 1024);
        e = bfk_sum_probe(n, d_cell, d_value, n_cells, lds ? 1 : 0, d_limbs, grid, nullptr);
    }
    if (e == hipSuccess) e = bfk_sum_resolve(d_limbs, d_out, n_cells, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, (size_t) n_cells * 4, hipMemcpyDeviceToHost);
    (void) hipFree(d_cell);
    (void) hipFree(d_value);
    (void) hipFree(d_out);
    (void) hipFree(d_limbs);
    if (e != hipSuccess) return fail(BF_ERR_DEVICE, "bf_exact_sum: %s", hipGetErrorString(e));
    return BF_OK;
}

// ---- device-side queries (include/beifong_hip.h: "Plugin-level queries") -------------------------------------------------
// Both forms of every query go through BF_ENTER and are ordered like a render: they wait for the handle's last work on another
// stream (order_after_last) and record themselves as its last work (mark_last), so a later endpoint update or mesh transform
// cannot overwrite a table a query still reads.  Queries only read the scene, so an open rolling sequence stays open.
enum { kQueryEvalPdf = 0, kQuerySample = 1, kQueryEmitter = 2, kQuerySensor = 3 };
static constexpr uint64_t kQueryMax = 0xffffffffull;      // queries per call: the launch grid is (n + 255) / 256 blocks

static bf_status query_device(const bf_scene *scene, int op, uint64_t n, const uint32_t *materials, uint32_t emitter,
                              const float *in, float *out, void *stream_, const char *who) {
    if (!scene) return fail(BF_ERR_INVALID, "%s: null scene", who);
    const bool per_material = op == kQueryEvalPdf || op == kQuerySample;
    if (n && (!in || !out || (per_material && !materials))) return fail(BF_ERR_INVALID, "%s: null pointer with n = %llu", who, (unsigned long long) n);
    if (n > kQueryMax) return fail(BF_ERR_INVALID, "%s: %llu queries (at most %llu per call)", who, (unsigned long long) n, (unsigned long long) kQueryMax);
    BF_ENTER(scene);
    if (op == kQueryEmitter) {
        if (emitter >= scene->ends.emitter_types.size())
            return fail(BF_ERR_INVALID, "%s: emitter %u out of range (%zu emitters)", who, emitter, scene->ends.emitter_types.size());
        const uint32_t t = scene->ends.emitter_types[emitter];
        if (t != BF_EMITTER_SPOT && t != BF_EMITTER_AREA && t != BF_EMITTER_POINT)
            return fail(BF_ERR_UNSUPPORTED, "%s: emitter %u is a transmitter (type %u): no probe", who, emitter, t);
    }
    if (op == kQuerySensor) {
        const uint32_t t = scene->ends.sensor_host.type;
        if (t != BF_SENSOR_FLUXMETER && t != BF_SENSOR_PERSPECTIVE && t != BF_SENSOR_IRRADIANCEMETER && t != BF_SENSOR_RADIANCEMETER)
            return fail(BF_ERR_UNSUPPORTED, "%s: the scene's endpoint is a receiver (type %u): no probe", who, t);
    }
    if (n == 0) return BF_OK;
    hipStream_t stream = (hipStream_t) stream_;
    bf_status st = order_after_last(scene, stream);
    if (st != BF_OK) return st;
    HIP_TRY(bfk_launch_query(op, &scene->d, n, materials, emitter, in, out, stream));
    return mark_last(scene, stream);
}

// host form: stage the rows, run the device form on the null stream, copy back and wait for that stream
static bf_status query_host(const bf_scene *scene, int op, uint64_t n, const uint32_t *materials, uint32_t emitter, const float *in,
                            uint32_t in_floats, float *out, uint32_t out_floats, const char *who) {
    const bool per_material = op == kQueryEvalPdf || op == kQuerySample;
    // the refusals of the device form first (it launches nothing for n = 0), then the material indices, which only the host sees
    bf_status st = query_device(scene, op, 0, materials, emitter, in, out, nullptr, who);
    if (st != BF_OK) return st;
    if (n && (!in || !out || (per_material && !materials))) return fail(BF_ERR_INVALID, "%s: null pointer with n = %llu", who, (unsigned long long) n);
    if (n > kQueryMax) return fail(BF_ERR_INVALID, "%s: %llu queries (at most %llu per call)", who, (unsigned long long) n, (unsigned long long) kQueryMax);
    if (per_material)
        for (uint64_t i = 0; i < n; ++i)
            if (materials[i] >= scene->ends.n_materials)
                return fail(BF_ERR_INVALID, "%s: query %llu: material %u out of range (%u materials)", who, (unsigned long long) i, materials[i],
                            scene->ends.n_materials);
    if (n == 0) return BF_OK;
    DeviceGuard on_device(scene->device);
    float *d_in = nullptr, *d_out = nullptr;
    uint32_t *d_mat = nullptr;
    hipError_t e = hipMalloc((void **) &d_in, n * in_floats * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **) &d_out, n * out_floats * sizeof(float));
    if (e == hipSuccess && per_material) e = hipMalloc((void **) &d_mat, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemcpy(d_in, in, n * in_floats * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess && per_material) e = hipMemcpy(d_mat, materials, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        st = query_device(scene, op, n, d_mat, emitter, d_in, d_out, nullptr, who);
        if (st == BF_OK) e = hipMemcpyAsync(out, d_out, n * out_floats * sizeof(float), hipMemcpyDeviceToHost, nullptr);
        if (st == BF_OK && e == hipSuccess) e = hipStreamSynchronize(nullptr);
    }
    (void) hipFree(d_in);
    (void) hipFree(d_out);
    if (d_mat) (void) hipFree(d_mat);
    if (st != BF_OK) return st;
    if (e != hipSuccess) return fail(BF_ERR_DEVICE, "%s: %s", who, hipGetErrorString(e));
    return BF_OK;
}

bf_status bf_bsdf_eval_pdf_device(const bf_scene *scene, uint64_t n, const uint32_t *materials, const float *wi_wo, float *out,
                                  void *stream) {
    return query_device(scene, kQueryEvalPdf, n, materials, 0, wi_wo, out, stream, __func__);
}
bf_status bf_bsdf_eval_pdf(const bf_scene *scene, uint64_t n, const uint32_t *materials, const float *wi_wo, float *out) {
    return query_host(scene, kQueryEvalPdf, n, materials, 0, wi_wo, 6, out, 2, __func__);
}
bf_status bf_bsdf_sample_device(const bf_scene *scene, uint64_t n, const uint32_t *materials, const float *wi_u, float *out, void *stream) {
    return query_device(scene, kQuerySample, n, materials, 0, wi_u, out, stream, __func__);
}
bf_status bf_bsdf_sample(const bf_scene *scene, uint64_t n, const uint32_t *materials, const float *wi_u, float *out) {
    return query_host(scene, kQuerySample, n, materials, 0, wi_u, 6, out, 5, __func__);
}
bf_status bf_emitter_sample_direction_device(const bf_scene *scene, uint32_t emitter, uint64_t n, const float *in, float *out,
                                             void *stream) {
    return query_device(scene, kQueryEmitter, n, nullptr, emitter, in, out, stream, __func__);
}
bf_status bf_emitter_sample_direction(const bf_scene *scene, uint32_t emitter, uint64_t n, const float *in, float *out) {
    return query_host(scene, kQueryEmitter, n, nullptr, emitter, in, 5, out, 8, __func__);
}
bf_status bf_sensor_sample_ray_device(const bf_scene *scene, uint64_t n, const float *in, float *out, void *stream) {
    return query_device(scene, kQuerySensor, n, nullptr, 0, in, out, stream, __func__);
}
bf_status bf_sensor_sample_ray(const bf_scene *scene, uint64_t n, const float *in, float *out) {
    return query_host(scene, kQuerySensor, n, nullptr, 0, in, 4, out, 9, __func__);
}

// the ray queries on device rays: bf_trace_any / bf_ray_intersect's kernel as it is, on the caller's stream
static bf_status trace_device(const bf_scene *scene, uint64_t n, const float *rays, int any_hit, uint8_t *out_hit, float *out_si,
                              uint32_t *out_prim, uint32_t *out_shape, void *stream_, const char *who) {
    if (!scene) return fail(BF_ERR_INVALID, "%s: null scene", who);
    if (n && (!rays || (any_hit ? !out_hit : !out_si))) return fail(BF_ERR_INVALID, "%s: null pointer with n = %llu", who, (unsigned long long) n);
    BF_ENTER(scene);
    if (n == 0) return BF_OK;
    hipStream_t stream = (hipStream_t) stream_;
    bf_status st = order_after_last(scene, stream);
    if (st != BF_OK) return st;
    HIP_TRY(bfk_launch_trace(&scene->d, n, rays, any_hit, nullptr, out_prim, out_shape, nullptr, out_hit, out_si, stream));
    return mark_last(scene, stream);
}
bf_status bf_ray_intersect_device(const bf_scene *scene, uint64_t n, const float *rays, float *out_si, uint32_t *out_prim,
                                  uint32_t *out_shape, void *stream) {
    return trace_device(scene, n, rays, 0, nullptr, out_si, out_prim, out_shape, stream, __func__);
}
bf_status bf_trace_any_device(const bf_scene *scene, uint64_t n, const float *rays, uint8_t *out_hit, void *stream) {
    return trace_device(scene, n, rays, 1, out_hit, nullptr, nullptr, nullptr, stream, __func__);
}

bf_status bf_eval_microfacet(int op, uint32_t distribution, float alpha_u, float alpha_v, uint32_t sample_visible, uint64_t n,
                             const float *in, float *out) {
    if (op < 0 || op > 3) return fail(BF_ERR_INVALID, "bf_eval_microfacet: op %d (0 eval, 1 pdf, 2 smith_g1, 3 sample)", op);
    if (distribution != BF_MF_BECKMANN && distribution != BF_MF_GGX)
        return fail(BF_ERR_INVALID, "bf_eval_microfacet: distribution %u (BF_MF_BECKMANN or BF_MF_GGX)", distribution);
    if (n && (!in || !out)) return fail(BF_ERR_INVALID, "bf_eval_microfacet: null pointer with n = %llu", (unsigned long long) n);
    if (n > kQueryMax) return fail(BF_ERR_INVALID, "bf_eval_microfacet: %llu queries (at most %llu per call)", (unsigned long long) n,
                                   (unsigned long long) kQueryMax);
    if (n == 0) return BF_OK;
    float *d_in = nullptr, *d_out = nullptr;
    hipError_t e = hipMalloc((void **) &d_in, n * 8 * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void **) &d_out, n * 4 * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_in, in, n * 8 * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = bfk_launch_microfacet(op, distribution, alpha_u, alpha_v, sample_visible, n, d_in, d_out, nullptr);
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n * 4 * sizeof(float), hipMemcpyDeviceToHost, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    (void) hipFree(d_in);
    (void) hipFree(d_out);
    if (e != hipSuccess) return fail(BF_ERR_DEVICE, "bf_eval_microfacet: %s", hipGetErrorString(e));
    return BF_OK;
}

}  // extern "C"
