// What bf_api.cpp, bf_render.cpp, bf_mesh.cpp, bf_pose.cpp and bf_endpoints.cpp share: the scene handle, its guards and the few functions of each file the others call.
// Internal to libbeifong_hip.so: the functions and guards declared here have hidden visibility (the C ABI is include/beifong_hip.h alone).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <functional>
#include <memory>
#include <vector>

#include "bf_build.h"
#include "bf_bvh.h"
#include "bf_converge.h"
#include "bf_device.h"
#include "bf_launch.h"
#include "bf_wavefront.h"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess) return fail(BF_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

inline int32_t bfd_no_node() { return INT32_MIN; }
constexpr size_t kTriPad = 4;      // float4 rows of padding behind the triangle array (read by no kernel; part of the geometry layout)

// The big read-only arrays of a scene (BVH nodes, triangles, normals, texture coordinates): shared by a scene and its
// clones (bf_scene_clone), freed with the last of them.
struct bf_geometry {
    std::vector<void *> owned;
    // vertex updates (bf_scene_update_vertices): what every mesh shape was created with, and the device corner
    // table built from it at the first update of any handle that shares these arrays (one uint4 per triangle slot in leaf order:
    // the slot's three vertex indices within its shape, then the shape).  `indices` goes once the corner table holds it, except
    // for a mesh with vertex normals: its normal index (below) may still have to be built from it.
    struct MeshTopo {
        uint32_t n_vertices = 0, n_faces = 0, prim0 = 0;
        bool has_normals = false;
        std::vector<uint32_t> indices;
    };
    std::vector<MeshTopo> topo;            // per shape (non-mesh shapes: empty)
    uint4 *corners = nullptr;
    // recomputed normals (BF_NORMALS_RECOMPUTE): the inverted index of one shape's faces, built at the first
    // recomputation of the shape by any handle that shares this geometry: offset[n_vertices + 1], and per incident corner one uint4
    // (the face's three vertex indices, then the corner number), sorted by face.  Per vertex and face, not per slot:
    // bf_scene_rebuild_bvh hands the same objects to the geometry it makes.
    struct NormalIndex {
        uint32_t *offset = nullptr;
        uint4 *entries = nullptr;
        ~NormalIndex() {
            if (offset) (void) hipFree(offset);
            if (entries) (void) hipFree(entries);
        }
    };
    std::vector<std::shared_ptr<const NormalIndex>> normal_index;      // per shape, null until built
    ~bf_geometry() {
        for (void *p : owned) (void) hipFree(p);
    }
};

// Developer overrides, read from the environment ONCE, when a scene is created; clones inherit them.
struct bf_tunables {
    uint32_t pool = 1u << 24;                // BF_WF_POOL
    int64_t tail = -1;                       // BF_WF_TAIL (-1: by pool size)
    uint32_t trace_refill = bfd::kTraceRefill, trace_stragglers = bfd::kTraceStragglers;
    uint32_t shade_chain = bfd::kShadeChain, row_jobs = bfd::kTailRowJobs;
    int shade_waves = 3, trace_waves = 5, tail_waves = 3;
    int gen_waves = 4;                       // waves per SIMD of the launches of wf_shade that start paths (first / wake), where a four-wave build exists
                                             // and four workgroups' LDS fit a CU (bf_render.cpp: wf_setup); BF_SHADE_WAVES set: that budget, like every shading launch
    unsigned tail_spread = 1, tail_blocks = 0;
    int tail_share = -1;                     // BF_TAIL_SHARE: waves per batch in a stand-alone render's tail (-1: by pool size)
    bool allow_plan = true;                  // BF_WF_SYNC=1 turns launch plans off
    uint32_t roll_iters = 0;                 // BF_ROLL_ITERS: bounce iterations per call of a rolling sequence (0: adaptive)
    uint32_t roll_live = 0;                  // BF_ROLL_LIVE: a rolling call stops iterating once at most this many slots are alive (0: max(1.5 x 2^20, main slots / 4))
    bool no_wide = false, quant = false;
    int wide_rows_log = -1;
    bool lean = true;                        // BF_LEAN=0: never use the kernels' lean variants (bf_device.h: kLean)
    bool tab_cache = true;                   // BF_TAB_CACHE=0: materials / rectangles stay in device memory (no LDS copies)
    bool shade_split = false;                // BF_SHADE_SPLIT=1: wf_shade walks the alive masks twice: slots without a real hit first, real hits second (measured: no net gain)
    uint32_t chain_min = 16;                 // BF_CHAIN_MIN: resolved real hits chain only while at least this many lanes hold one (0: always)
    uint32_t grid_share = 3;                 // BF_GRID_SHARE: small pools (< grid_small slots) of handles that roll side by side launch 1 / min(peers, this) of the persistent grids (0 / 1: off)
    uint32_t grid_small = 1u << 22;          // BF_GRID_SMALL
    bool roll_join = true;                   // BF_ROLL_JOIN=0: bf_scene_update_endpoints flushes an open rolling sequence (round 3's behaviour)
    uint32_t debug_surv_batches = 0;         // BF_DEBUG_SURV_BATCHES (tests): size of the survivor area in batches, sizing rule off
};

// The skin of one mesh shape (bf_scene_set_skin): rest pose and four bone slots per vertex in ONE device block, never
// written after it is made.  Handles share it through MeshState::skins (a clone copies the pointers; bf_scene_set_skin replaces this
// handle's pointer alone: copy on write); the block goes with the last of them.
struct __attribute__((visibility("hidden"))) MeshSkin {
    uint32_t n_bones = 0, n_vertices = 0;
    void *block = nullptr;                // device: what the four pointers below point into
    const float4 *weight = nullptr;       // [n_vertices]: w0..w3
    const uint4 *index = nullptr;         // [n_vertices]: i0..i3, each < n_bones
    const float *rest_pos = nullptr;      // [n_vertices][3]
    const float *rest_nrm = nullptr;      // [n_vertices][3], or null: the mesh has no vertex normals
    // what the bound on the posed coordinates is derived from (bf_pose.cpp: skin_bound)
    float rest_abs[3] = {0.f, 0.f, 0.f};  // max |rest coordinate| per axis
    double weight_sum = 0.0;              // largest float64 sum of a weight row (validated: within 1e-3 of 1)
    float pivot_min = 1.f;                // smallest over the rows of the row's largest weight (skin_bound_dq's kappa; >= 0.24975 by the row sums)
    std::vector<uint8_t> bone_used;       // [n_bones]: some vertex gives the bone a non-zero weight
    ~MeshSkin() {
        if (block) (void) hipFree(block);
    }
};

// The morph targets of one mesh shape (bf_scene_set_morph): rest pose and dense per-target deltas in ONE device block,
// never written after it is made; held and shared as MeshSkin is, through MeshState::morphs.
struct __attribute__((visibility("hidden"))) MeshMorph {
    uint32_t n_targets = 0, n_vertices = 0;
    void *block = nullptr;                // device: what the four pointers below point into
    const float *rest_pos = nullptr;      // [n_vertices][3]
    const float *rest_nrm = nullptr;      // [n_vertices][3], or null: the mesh has no vertex normals
    const float *dpos = nullptr;          // [n_targets][n_vertices][3]
    const float *dnrm = nullptr;          // [n_targets][n_vertices][3], or null: the rest normals are copied
    // what the bound on the morphed coordinates is derived from (bf_pose.cpp: morph_extent)
    float rest_abs[3] = {0.f, 0.f, 0.f};  // max |rest coordinate| per axis
    std::vector<float> delta_abs;         // [n_targets][3]: max |delta coordinate| per target and axis
    ~MeshMorph() {
        if (block) (void) hipFree(block);
    }
};

// "The meshes of this handle have moved" (DESIGN.md 6d): the state bf_mesh.cpp keeps per handle, each flag's meaning stated here alone.
// Every moving call is ABSOLUTE: from the BASE rows (as created, until a vertex update rewrites them) to the rows bf_scene::d renders.
struct __attribute__((visibility("hidden"))) MeshState {
    // the base rows; all null until the handle's first move (own_geometry sets the three together), then never null again
    float4 *tris0 = nullptr, *nodes0 = nullptr, *wnodes0 = nullptr;
    float4 *normals0 = nullptr;          // the base vertex normals, once d.normals is the handle's own array (own_normals)
    bool geom_private = false;           // d.tris / d.nodes / d.wnodes / d.qnodes are this handle's own moved copies, not the arrays shared with clones
    bool base_private = false;           // tris0 is this handle's own allocation, so a vertex update may write it (false: it READS the shared rows)
    bool normals_private = false;        // d.normals is this handle's own array (copy on write, as geom_private for the rest)
    bool normals0_private = false;       // normals0 is this handle's own allocation, so a vertex update with normals may write it
    bool normals_moved = false;          // d.normals holds normals a rigid table has turned: a translation restores normals0 first
    bool deformed = false;               // nodes0 / wnodes0 no longer bound the base rows (vertex update, rebuild under a pose): only their topology is read, and translations refit too
    int pose_kind = 0;                   // the latest pose, run again after a vertex update: 0 none, 1 a translation, 2 a rigid table
    std::vector<float> pose_xf;          // that pose as bfk_launch_rigid reads it (16 floats per shape)
    float origin_scale_built = 0.f;      // ray-origin bound the BVH boxes were padded for (bf_bvh.h): raised by moves, never lowered
    // the refit's state, built on the handle's first transform (nothing of it costs bf_scene_create anything)
    struct Refit {
        bool ready = false;
        bool have_boxes = false;                 // xf and mesh_box exist (they survive bf_scene_rebuild_bvh: neither depends on the slot order)
        std::vector<uint32_t> off4, off16;       // level d of the four- / sixteen-wide tree: [off[d], off[d + 1]) of lvl4 / lvl16
        uint32_t *lvl4 = nullptr, *lvl16 = nullptr;
        float4 *ubox4 = nullptr, *ubox16 = nullptr;      // unpadded bounds of every child record (two float4 each)
        float *xf = nullptr;                     // device: 16 floats per shape (bfk_launch_rigid)
        std::vector<float> mesh_box;             // per shape: lo.xyz, hi.xyz of its base triangles (inverted: none)
    } refit;
    // motion / deform batches: the geometry versions of a batch's renders, MotionLayout::rows float4 rows each.  Never shared with
    // clones, grown on demand; stream-ordered behind the previous call's renders like every write of the handle (order_after_last)
    float4 *arena = nullptr;
    size_t arena_cap = 0;                        // float4 rows allocated
    // the versions the last batch left in the arena, for bfdbg_scene_read_tree: 0 if that batch was chunked (the arena then holds
    // its last chunk only), failed, or a rebuild has changed the layout since
    uint32_t batch_versions = 0;
    size_t batch_rows = 0;                       // float4 rows per version of that batch
    // the device forms' violation counter ([0] slots refused, [1] a refused shape + 1), its pinned mirror and the event behind the
    // copy that follows every device-form gather
    uint32_t *bad = nullptr, *bad_host = nullptr;
    hipEvent_t bad_ev = nullptr;
    mutable bool bad_pending = false;
    mutable uint32_t bad_reported = 0;           // of the device count, how much has been reported already
    // the host form's upload buffer (pinned + device mirror), grown on demand; vtx_ev: behind the gather that read it last
    void *vtx_host = nullptr, *vtx_dev = nullptr;
    size_t vtx_cap = 0;
    hipEvent_t vtx_ev = nullptr;
    // skins (bf_scene_set_skin) and morph targets (bf_scene_set_morph), bf_pose.cpp's: per shape, empty until the first one is
    // attached; shared with clones taken afterwards.  pose_vtx: where bf_skin_vertices_kernel or bf_morph_vertices_kernel writes the
    // posed vertices (and normals) of a pose or of a batch chunk, for the gather to read; the handle's own, grown on demand, never shrunk
    std::vector<std::shared_ptr<const MeshSkin>> skins;
    std::vector<std::shared_ptr<const MeshMorph>> morphs;
    float *pose_vtx = nullptr;
    size_t pose_vtx_cap = 0;                     // bytes
    // normal modes (bf_scene_set_normal_mode): BF_NORMALS_* per shape, empty until the first call (every shape BF_NORMALS_GIVEN);
    // a clone copies them.  nrm_vtx: where bf_vertex_normals_kernel writes the normals of an update or of a batch chunk, for the
    // gather to read; the posed-vertex scratch's rules
    std::vector<uint8_t> normal_mode;
    float *nrm_vtx = nullptr;
    size_t nrm_vtx_cap = 0;                      // bytes
    bool recomputes(uint32_t shape) const { return shape < normal_mode.size() && normal_mode[shape] == BF_NORMALS_RECOMPUTE; }
    // skin modes (bf_scene_set_skin_mode): BF_SKIN_* per shape, held as the normal modes are (empty: every shape BF_SKIN_LINEAR; a
    // clone copies them); kept apart from `skins`, so a mode outlives the skin it was set for.  Read by every call that takes bones
    std::vector<uint8_t> skin_mode;
    bool skins_dq(uint32_t shape) const { return shape < skin_mode.size() && skin_mode[shape] == BF_SKIN_DUAL_QUATERNION; }
    // velocity modes (bf_scene_set_velocity_mode): BF_VELOCITY_* and the time step per shape, held as the normal modes
    // are (empty: every shape BF_VELOCITY_TWIST; a clone copies them and the rows).  vel: the velocity rows the handle's own renders
    // read under a range-rate table, three float4 per triangle slot (bf_velocity.h), allocated by the first mode other than
    // BF_VELOCITY_TWIST and zero until a field is given or a move differences it.  vel_prev: the rendered triangle rows as they were
    // before the move in progress (scratch).  vel_tab: device [n_shapes] (mode bits, dt), what bf_velocity_diff_kernel reads.
    // batch_vel: the versions of the last batch carried velocity rows (MotionLayout).  All four go with the handle.
    std::vector<uint8_t> vel_mode;
    std::vector<float> vel_dt;
    float4 *vel = nullptr, *vel_prev = nullptr;
    float2 *vel_tab = nullptr;
    bool batch_vel = false;
    uint32_t velocity_mode(uint32_t shape) const { return shape < vel_mode.size() ? vel_mode[shape] : (uint32_t) BF_VELOCITY_TWIST; }
    bool velocities() const {          // some shape is in BF_VELOCITY_VERTEX or BF_VELOCITY_DIFFERENCE
        for (uint8_t v : vel_mode)
            if (v != BF_VELOCITY_TWIST) return true;
        return false;
    }
    bool differences() const {         // some shape is in BF_VELOCITY_DIFFERENCE
        for (uint8_t v : vel_mode)
            if (v == BF_VELOCITY_DIFFERENCE) return true;
        return false;
    }

    // what to read as the base rows: the handle's own once it has moved, else the arrays it renders (a clone's snapshot included)
    struct Base { const float4 *tris, *nodes, *wnodes, *normals; };
    Base base(const bfd::DScene &d) const {
        return {tris0 ? tris0 : d.tris, tris0 ? nodes0 : d.nodes, tris0 ? wnodes0 : d.wnodes, normals0 ? normals0 : d.normals};
    }
    // byte sizes of the arrays of n_tris triangles, n_nodes Node4 and wide_nodes Node16 (0: no such tree); quantised nodes: nodes / 2
    struct Bytes { size_t tris, normals, nodes, wnodes; };
    static Bytes bytes(uint32_t n_tris, uint32_t n_nodes, size_t wide_nodes) {
        return {((size_t) n_tris * bfd::kTriStride + kTriPad) * sizeof(float4), (size_t) n_tris * 3 * sizeof(float4), (size_t) n_nodes * 8 * sizeof(float4),
                wide_nodes * 32 * sizeof(float4)};
    }
    static Bytes bytes(const bfd::DScene &d) { return bytes(d.n_tris, d.n_nodes, d.wnodes ? d.n_wnodes : 0); }
    // copy on write of the rendered normals: d.normals becomes the handle's own array (the caller fills it), the old one stays as normals0
    bf_status own_normals(bfd::DScene &d, std::vector<void *> &owned, const char *who);
    // after bf_scene_rebuild_bvh's swap: the permuted base arrays (all null unless the handle was posed) and what follows from them
    void reset_after_rebuild(float4 *tris0_, float4 *nodes0_, float4 *wnodes0_, float4 *normals0_);
    // arena, violation counter and upload buffer go with the handle (the base arrays and the refit's are on bf_scene::owned)
    ~MeshState();
};

// Everything a render of this handle leaves behind for the next one (bf_render.cpp): the path pool and its read-back buffers, the
// launch statistics, the open rolling sequence, the learned launch plan, the live-count feedback and the stream order between calls.  Each field's meaning is stated here alone.  Renders take const bf_scene *, hence the keyword on bf_scene::run.
struct __attribute__((visibility("hidden"))) RenderState {
    // ---- the path pool, allocated on first use and grown on demand (wf_ensure) ----
    bfd::WF wf{};
    std::vector<void *> pool;                   // every device allocation of the pool (masks, ring and offsets included)
    unsigned long long *masks = nullptr;        // the batch masks wf.m_* point into
    bfd::DRoll *roll_ring = nullptr;            // device [kRollRing]: the descriptors of a rolling sequence's renders
    float4 *roll_offsets = nullptr;             // device [kRollRing]: mesh offset of every render of the sequence
    unsigned long long *counters = nullptr;     // device CTR_* (bf_device.h), allocated with the handle; the last two are the sticky guard words
    // pinned read-back: word [0] = n_live[it] of a synchronous drive loop, 64-bit words [1], [2] = the guard words a plan's feedback carries
    uint32_t *host = nullptr;
    hipEvent_t event = nullptr;                 // behind the copy into host[0]; also the cross-stream hand-over (hand_over)
    // ---- launch statistics of the last stats render / rolling sequence (bf_stats) ----
    std::vector<hipEvent_t> timing;             // event pool for per-kernel timing: pair k = events 2k, 2k + 1
    std::vector<int> ev_kind;                   // kind of every recorded pair: 0 trace, 1 shade, 2 tail
    float ms[3] = {0, 0, 0};                    // trace, shade, tail
    uint32_t iters = 0, trace_launches = 0, tail_launches = 0, shade_launches = 0;
    uint32_t last_variant = 0;                  // BF_VARIANT_* of the latest render (bf_stats.kernel_variant)
    int gen_waves_last = 0;                     // waves per SIMD of the build the latest generation launch (first / wake) ran (bfdbg_scene_generation_waves)
    // ---- the AOV table of the handle (bf_scene_set_aovs; BF_FLAG_AOV) and the side rows its launches carry the values in ----
    struct Aov {
        uint32_t n = 0;                          // entries; 0: no table
        uint32_t types[BF_MAX_AOVS] = {};        // BF_AOV_*, in channel order
        float *rows = nullptr;                   // device side rows (bf_device.h: AovCtx), allocated by the first AOV launch, grown on demand
        uint64_t rows_floats = 0;
    } aov;
    // ---- the limb cells of the handle's BF_FLAG_EXACT_SUM launches (bf_sum.h): n_chan_all cells of 72 bytes, allocated by the first such
    // launch, grown on demand, freed with the handle; zeroed ahead of a launch's first kernel, resolved into hist_dev behind its last ----
    struct Sum {
        void *limbs = nullptr;
        uint64_t cells = 0;
    } sum;
    // ---- rolling sequence (bf_render_device with BF_FLAG_ROLLING, bf_scene_flush): see wf_roll_render ----
    struct Roll {
        bool open = false;
        uint32_t count = 0;                      // renders issued since the sequence was opened
        uint32_t it = 0;                         // bounce-iteration counter (mask parity runs on across calls)
        bf_launch shape;                         // launch of the first render: later ones may differ in seed / path_offset only
        bfd::DLaunch lp;                         // device launch of the sequence (n_paths = supply so far)
        hipStream_t stream = nullptr;
        bool count_nodes = false, timed = false;
        uint32_t per_call = 1;                   // renders every call adds (bf_render_batch_device: the batch size)
        bool offsets = false;                    // the renders carry mesh offsets (batched calls with moving meshes)
        float dmax = 0.f;                        // largest |offset component| so far (box slack of the SHIFT traversal)
        uint32_t window = 1;                     // renders of the LDS histogram window
        uint32_t iters = 0;                      // bounce iterations per call (adapted from the live counts)
        uint32_t flush_iters = 0;                // planned bounce iterations of a flush before its tail (learned)
        uint32_t flush_live = 0;                 // slots alive at the flush's tail (learned: sizes its grid)
        bool multi = false;                      // the endpoints moved between the renders of the sequence (kMulti kernels from then on)
    } roll;
    // Launch plan learned from the previous render of the same shape (wf_render): how many bounce iterations precede the tail and
    // how many slots are then alive.  With a plan the whole render is enqueued without a host round trip.
    struct Plan {
        bool valid = false;
        uint64_t n_paths = 0;
        uint32_t mode = 0, max_depth = 0, n_slots = 0, tail_max = 0;
        uint32_t iters = 0, tail_live = 0;
    } plan;
    // The live-count feedback channel: a planned drive loop never waits for n_live, it posts a copy of the counts behind an event
    // and whoever drives the handle next takes them if they have landed (never waiting) and learns from them.  One copy is in
    // flight at most: a post while one is pending is skipped.  `owner` says whose counts they are; it is written by post() and read
    // by take() alone, that is only while `pending` is set, so nothing has to reset it when the counts are dropped.
    struct Feedback {
        enum Owner { kNone, kPlan, kRollCall, kRollFlush };      // wf_render's plan, a call of a rolling sequence, its flush
        uint32_t *counts = nullptr;              // pinned [kWfMaxIter + 2]
        volatile unsigned long long *guards = nullptr;   // the two guard words of a kPlan post (RenderState::host, words [1], [2])
        hipEvent_t event = nullptr;
        bool pending = false;
        uint32_t n = 0;                          // counts in flight
        Owner owner = kNone;
        struct Landed {
            const uint32_t *counts;
            uint32_t n;
            Owner owner;                         // kNone: nothing has landed
        };
        // src[0 .. n) -> counts behind `stream` (guards_src: and the two sticky guard words); nothing if a copy is in flight already
        hipError_t post(const uint32_t *src, uint32_t n, Owner owner, hipStream_t stream, const unsigned long long *guards_src = nullptr);
        Landed take();                           // the counts, once, if their copy has completed
        void drop() { pending = false; }         // whatever is in flight is nobody's
        // index of the first count <= threshold (n: none)
        static uint32_t first_at_most(const uint32_t *counts, uint32_t n, uint32_t threshold);
    } fb;
    // Stream order between the successive uses of the handle: order_after_last / mark_last
    struct LastUse {
        hipStream_t stream = nullptr;
        hipEvent_t done = nullptr;               // recorded behind the handle's latest work
        bool has = false;
        hipError_t wait() const { return has ? hipEventSynchronize(done) : hipSuccess; }      // the host waits for that work
    } last;
    // bf_render_converge_device, allocated on first use: the rounds' scratch histograms (double-buffered, [R][channels]
    // each), the statistic kernels' hand-over words, the pinned ring their results land in and one event per round in flight
    struct Converge {
        static constexpr uint32_t kRing = 4;     // slot r % kRing: at most two rounds are in flight
        float *scratch[2] = {nullptr, nullptr};
        size_t cap = 0;                          // floats per scratch buffer
        bfd::ConvWork *ws = nullptr;             // device
        bfd::ConvResult *ring = nullptr;         // pinned [kRing]
        hipEvent_t ev[2] = {nullptr, nullptr};   // behind round r's statistic: ev[r & 1]
    } conv;
    // pool, pinned buffers, events, timing events, counters and the converge state go with the handle
    ~RenderState();
};

// The endpoint tables of a handle (bf_endpoints.cpp): rectangles, shapes, emitters, materials and the sensor record in ONE device block,
// the phased-array element tables, the class table, and everything the host derives from them (which kernel variant a render launches,
// what a launch is refused for).  Each field's meaning is stated here alone.  close_sequence takes const bf_scene *, hence the keyword on
// bf_scene::ends.
struct __attribute__((visibility("hidden"))) EndpointState {
    // The host image of a description's endpoint half (endpoints_flatten): the five tables as the kernels read them, and what the
    // profile needs that the tables do not carry.  apply() derives everything else from it.
    struct Image {
        std::vector<bfd::DRect> rects;
        std::vector<bfd::DShape> shapes;
        std::vector<bfd::DEmitter> emitters;     // velems of phased ones: the caller's host table until bind_arrays has run, the device copy then
        std::vector<bfd::DMaterial> materials;
        bfd::DSensor sensor;                     // (velems likewise)
        uint32_t n_tris = 0;                     // triangles of all mesh shapes
        uint32_t window_t = 0, window_f = 0;     // ADC window size (0: the whole ADC)
        uint32_t film_w = 1, film_h = 1;
        float c = 0.f, lambda_min = 0.f, lambda_max = 0.f;      // the physics band (bf_scene_desc::physics)
        float origin_scale = 0.f;                // largest |coordinate| of a rectangle corner, emitter or sensor position
    };
    // ---- the profile: set by apply() alone (shapes_host: by endpoints_create), copied by a clone ----
    uint32_t n_rects = 0, n_shapes = 0, n_emitters = 0, n_materials = 0;      // the tables' sizes, fixed when the handle is created
    std::vector<uint32_t> emitter_types;
    bool any_back_material = false;        // some twosided material has a second nested BSDF (general kernels)
    bool any_resample = false;             // some transmitter re-samples the path's wavelength (resample_freq: general kernels, DLaunch::resample)
    bfd::DSensor sensor_host;              // host copy of the device sensor record
    uint32_t film_w = 1, film_h = 1;       // the sensor's film (bf_sensor.film_width / film_height)
    uint32_t adc_t = 0, adc_f = 0;         // what a receive-mode launch bins into: the ADC's window, or the whole ADC
    std::vector<bfd::DShape> shapes_host;  // as created, whatever later updates bring: mesh triangles carry their shape's material / emitter index
    // ---- the tables on the device ----
    // One block holds the five tables: the home block (as created) whenever no rolling sequence is open, and every block of the pool.
    // bf_scene_update_endpoints writes the new tables into the next block of the pool instead of flushing an open sequence (the
    // renders issued so far keep reading theirs through the descriptor ring: bf_device.h: DRoll, kMulti).  The staging slot of an
    // update has the same layout.
    struct Layout {                          // byte offsets of the five tables within a block, 16-byte aligned
        size_t o_rects = 0, o_shapes = 0, o_emit = 0, o_mat = 0, o_sensor = 0, total = 0;
    } lay;
    char *home = nullptr;                    // device: the home block (lay.total bytes)
    size_t stride = 0;                       // bytes per block of the pool (lay.total rounded up to 256)
    char *pool = nullptr;                    // device: kRollRing blocks (allocated on first use)
    uint32_t next = 0;                       // next free block
    bool in_pool = false;                    // d->rects ... d->sensor point into the pool
    bfd::DScene *d = nullptr;                // the handle's kernel arguments, whose five table pointers move between home and pool
    // device copies of the phased-array element tables: one per emitter (nullptr if none) + the receiver's
    std::vector<float *> array_dev;
    std::vector<uint32_t> array_n;
    float *sensor_array_dev = nullptr;
    uint32_t sensor_array_n = 0;
    uint32_t *classes = nullptr;             // device: shape_class[n_shapes], the arrival table's twelve words or the range-rate table's
                                             // 8 + 12 n_shapes (room for any) once bf_scene_set_classes / bf_scene_set_arrival_classes /
                                             // bf_scene_set_range_rate_classes has given one (d->class_lo / class_hi)
    std::vector<uint32_t> rr_words;          // the range-rate table as installed, while that form is the handle's (else empty): what
                                             // velocity_stamp patches and copies again when a velocity mode or the rows' address changes

    void apply(const Image &img, bool tab_cache);      // every count and profile bit, here and in *d, from a flattened description (tab_cache: bf_tunables)
    void pack(const Image &img, char *blk) const;      // the five tables into a host block of this layout
    void point_at(const char *blk);                    // *d reads its tables from this device block (an empty table: a null pointer)
    bf_status claim(char **blk);                       // the next free block of the pool (the first claim allocates it)
    void joined() { ++next, in_pool = true; }          // ... which now holds the handle's tables
    // the last version becomes the home block's content again, behind `stream`; the pointers are home before the copy can fail
    bf_status go_home(hipStream_t stream);
    // home block, pool, element tables and class table go with the handle
    ~EndpointState();
};

struct bf_scene {
    bfd::DScene d;
    bf_tunables tun;
    std::shared_ptr<bf_geometry> geom;     // nodes / wnodes / tris / normals / uvs as created
    // handles that render the SAME triangle / node arrays hold the same token (a clone that took its own snapshot of a
    // translated scene does not): bf_scene_translate_meshes copies on write only while the token is shared
    std::shared_ptr<char> geom_token;
    // handles cloned from one another are meant to be in flight together (one per stream): how many of them have a rolling sequence
    // open right now — small pools then launch a share of the persistent grids each (wf_setup: grid_share)
    std::shared_ptr<std::atomic<int>> peers_rolling;
    // one host thread at a time per handle (the handle owns the path pool its render's state lives in)
    mutable std::atomic_flag busy = ATOMIC_FLAG_INIT;
    std::vector<void *> owned;             // this handle's own allocations (spill columns, private geometry)
    bf_scene_info info;
    int device = 0;
    int n_cus = 256;
    MeshState mesh;                        // everything about moved meshes (bf_mesh.cpp, bf_pose.cpp)
    mutable RenderState run;               // everything about renders (bf_render.cpp)
    mutable EndpointState ends;            // everything about the endpoint tables (bf_endpoints.cpp)
    // Pinned staging for small host tables that travel with a launch (batch seeds / mesh offsets, endpoint records):
    // a ring of slots, each with its own device mirror and an event recorded behind the copy, so the caller's arrays
    // and our stack locals are free again when the call returns and nothing blocks unless kStageSlots launches are in
    // flight on this scene.
    static constexpr int kStageSlots = 8;
    struct Stage {
        void *host = nullptr, *dev = nullptr;
        size_t cap = 0;
        hipEvent_t ev = nullptr;
        bool busy = false;
    };
    mutable Stage stage[kStageSlots];
    mutable int stage_next = 0;
};

#pragma GCC visibility push(hidden)      // from here on: internal to the library
// One host thread at a time per handle: the second one gets BF_ERR_INVALID instead of a race on the handle's pool.
struct BusyGuard {
    const bf_scene *s;
    bool ok;
    int prev_device = -1;
    // ... and every call runs on the handle's own device, whatever the caller's current one is (one host thread may
    // drive the handles of several GPUs: bf_render_sharded_device), restored on return
    explicit BusyGuard(const bf_scene *sc) : s(sc), ok(sc && !sc->busy.test_and_set(std::memory_order_acquire)) {
        if (ok) {
            int cur = -1;
            if (hipGetDevice(&cur) == hipSuccess && cur != sc->device && hipSetDevice(sc->device) == hipSuccess) prev_device = cur;
        }
    }
    ~BusyGuard() {
        if (prev_device >= 0) (void) hipSetDevice(prev_device);
        if (ok) s->busy.clear(std::memory_order_release);
    }
};
// the handle's device for the calls that allocate or launch before (or without) taking the busy flag
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int device) {
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess) prev = cur;
    }
    ~DeviceGuard() {
        if (prev >= 0) (void) hipSetDevice(prev);
    }
};
#define BF_ENTER_AS(scene, name)                                                                                          \
    BusyGuard busy_guard_(scene);                                                                                         \
    if (!busy_guard_.ok)                                                                                                  \
        return fail(BF_ERR_INVALID, "%s: the scene handle is in use by another host thread (one call at a time per handle; " \
                                    "bf_scene_clone gives every thread / stream its own)", name)
#define BF_ENTER(scene) BF_ENTER_AS(scene, __func__)      // (..._AS: for a body that several entries share)

// ---- bf_api.cpp's, called by the others and documented where they are defined (C names: those files are one extern "C" block each) ----
extern "C" {
bf_status fail(bf_status st, const char *fmt, ...);      // sets bf_last_error's text
bf_status stage_acquire(const bf_scene *sc, size_t bytes, bf_scene::Stage **out);
bf_status stage_commit(bf_scene::Stage *st, size_t bytes, hipStream_t stream);
bf_status stage_release_after(bf_scene::Stage *st, hipStream_t stream);

// ---- bf_render.cpp, called by the others ----
bf_status order_after_last(const bf_scene *scene, hipStream_t stream);
bf_status mark_last(const bf_scene *scene, hipStream_t stream);
bf_status close_sequence(const bf_scene *scene, hipStream_t stream);
bf_status check_classes(const bf_scene *scene, const bf_launch *launch, uint32_t n_renders);      // BF_FLAG_CLASSES refusals, before any device work
bf_status check_aov(const bf_scene *scene, const bf_launch *launch, uint32_t n_renders);          // BF_FLAG_AOV refusals, likewise
bf_status check_sum(const bf_scene *scene, const bf_launch *launch, uint32_t n_renders);          // BF_FLAG_EXACT_SUM refusals, likewise
bf_status render_locked(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, float *hist_dev, bf_path_record *records_dev,
                        void *stream_, bf_stats *stats_out, uint32_t geom_stride = 0);
void fill_stats(const bf_scene *scene, const unsigned long long *c, uint64_t n_paths, bf_stats *st);
void add_stats(bf_stats &a, const bf_stats &b);      // a += b (the chunks of a batch, the rounds of a converge call)
bf_status guard_error(unsigned long long lost, unsigned long long refused);
bf_status report_guards(const bf_scene *scene, unsigned long long lost, unsigned long long refused, const hipStream_t *async_on = nullptr);

// ---- bf_mesh.cpp, called by the others ----
// a device-form vertex update whose gather refused triangles: BF_ERR_DEVICE, once (wait: for the count; else only if it has landed)
bf_status deform_report(const bf_scene *scene, bool wait);
bf_status check_deform_shape(const bf_scene *scene, uint32_t shape, bool with_normals, const char *who, const bf_geometry::MeshTopo **topo_out);
// bf_scene_clone: if `src` has moved, `sc` (a copy of src's kernel arguments so far) takes its own snapshot of what src renders now
bf_status mesh_clone_snapshot(const bf_scene *src, bf_scene *sc);

// the velocity rows around a call that rewrites the rendered triangle rows (BF_VELOCITY_DIFFERENCE: the rows before the call are kept,
// and differenced against the rows after it into the handle's field); both do nothing while no shape is in that mode.  shape: the one
// shape the call moved (a vertex update, a pose: every other shape keeps its field), or kAllShapes (a transform, a translation)
constexpr uint32_t kAllShapes = UINT32_MAX;
bf_status velocity_before(bf_scene *scene, hipStream_t stream);
bf_status velocity_after(bf_scene *scene, uint32_t shape, hipStream_t stream);

// ---- bf_mesh.cpp, called by bf_pose.cpp (a pose ends in a device-form vertex update, a posed batch in a deform batch) ----
bf_status mesh_enter(const bf_scene *scene, hipStream_t stream);
bf_status update_vertices_locked(bf_scene *scene, uint32_t shape, const bf_geometry::MeshTopo &tp, const float *pos_dev, const float *nrm_dev,
                                 float bound, const float *box6, bool watch, hipStream_t stream);
// slice(k0, kc, hs): the copy `hs` of the source table becomes that of renders k0 .. k0 + kc; run once per chunk of the arena
using DeformSlice = std::function<bf_status(uint32_t k0, uint32_t kc, bfd::DDeformSrc *hs)>;
bf_status deform_versions(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, const std::vector<bfd::DDeformSrc> &src,
                          float bound, const float *to_world, const std::vector<uint8_t> &moves, float *hist_dev, bf_path_record *records_dev,
                          void *stream_, bf_stats *stats_out, const char *who, const DeformSlice &slice);
bf_status vertex_scratch(float *&buf, size_t &cap, size_t bytes, hipStream_t stream, const char *who, const char *what);
bf_status check_rigid_tables(const bf_scene *scene, const char *fn, uint32_t n_renders, uint32_t n_shapes, const float *to_world, uint8_t *moves);
// the preamble of the motion, deform, skin and morph batches: before the lock, and first thing behind it
bf_status check_batch_call(const char *fn, const char *kind, const bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const float *to_world,
                           uint32_t n_shapes, const float *hist_dev);
bool batch_ends_early(bf_scene *scene, const bf_launch *launch, uint32_t n_renders, const uint64_t *seeds, float *hist_dev,
                      bf_path_record *records_dev, void *stream_, bf_stats *stats_out, bf_status *st);

// ---- bf_endpoints.cpp, called by the others ----
// the endpoint half of a description (every refusal it has for one), before any device work
bf_status endpoints_flatten(const bf_scene_desc *desc, EndpointState::Image &img);
// bf_scene_create: the element tables and the home block of `sc` from `img`, and its profile; *bytes grows by the block's size
bf_status endpoints_create(bf_scene *sc, EndpointState::Image &img, uint64_t *bytes);
// bf_scene_clone: `sc` (whose kernel arguments are a copy of src's) takes src's profile and its own copies of src's tables
bf_status endpoints_clone(const bf_scene *src, bf_scene *sc);
// the handle's range-rate table (if that form is installed) with every shape's velocity mode and the address `rows` of the velocity
// rows its kernels are to read (nullptr: every shape as BF_VELOCITY_TWIST), copied to the device again in stream order
bf_status velocity_stamp(bf_scene *scene, const float4 *rows, hipStream_t stream);
}

#pragma GCC visibility pop
