// The render driver behind bf_render_device / bf_render_batch_device / bf_scene_flush / bf_scene_sync (include/beifong_hip.h): the
// wavefront control loops, launch plans, rolling sequences, guard words and statistics.  State: bf_scene::run (bf_scene.h: RenderState);
// kernels: bf_kernels.hip, bf_wavefront.hip.
#include "bf_scene.h"
#include "bf_sum.h"
#include "bf_variant.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

namespace {
// the kernels one render runs: the exact build, the fast-arithmetic one (BF_FLAG_FAST), the second-moment variants (BF_FLAG_MOMENT),
// the class variants (BF_FLAG_CLASSES), the AOV variants (BF_FLAG_AOV) or the exact-sum variants (BF_FLAG_EXACT_SUM)
struct Kernels {
    decltype(&bfk_launch_render) render;
    decltype(&bfk_wf_shade) shade;
    decltype(&bfk_wf_trace) trace;
    decltype(&bfk_launch_tail) tail;
    bfv::Feature feature;      // what bf_variant.h's selectors call the family, and whether its kernels are the fast object's
    bool fast;
};
const Kernels kExact = {bfk_launch_render, bfk_wf_shade, bfk_wf_trace, bfk_launch_tail, bfv::kPlain, false};
const Kernels kFast = {bfk_launch_render_fast, bfk_wf_shade_fast, bfk_wf_trace_fast, bfk_launch_tail_fast, bfv::kPlain, true};
const Kernels kMoment = {bfk_launch_render_moment, bfk_wf_shade_moment, bfk_wf_trace, bfk_launch_tail_moment, bfv::kFeatMoment, false};
const Kernels kClass = {bfk_launch_render_class, bfk_wf_shade_class, bfk_wf_trace, bfk_launch_tail_class, bfv::kFeatClass, false};
const Kernels kAov = {bfk_launch_render_aov, bfk_wf_shade_aov, bfk_wf_trace, bfk_launch_tail_aov, bfv::kFeatAov, false};      // (BF_FLAG_AOV: with none of the three above, check_aov)
const Kernels kSum = {bfk_launch_render_sum, bfk_wf_shade_sum, bfk_wf_trace, bfk_launch_tail_sum, bfv::kFeatSum, false};      // (BF_FLAG_EXACT_SUM: with none of the four above, check_sum)
// (BF_FLAG_MOMENT | BF_FLAG_FAST, and BF_FLAG_CLASSES with either, are refused before any kernel is chosen: check_launch)
const Kernels &kernels_for(uint32_t flags) {
    if (flags & BF_FLAG_EXACT_SUM) return kSum;
    return (flags & BF_FLAG_FAST) ? kFast : ((flags & BF_FLAG_MOMENT) ? kMoment : ((flags & BF_FLAG_CLASSES) ? kClass : ((flags & BF_FLAG_AOV) ? kAov : kExact)));
}
}  // namespace

// ---- RenderState's sub-objects (bf_scene.h) ----
hipError_t RenderState::Feedback::post(const uint32_t *src, uint32_t n_, Owner owner_, hipStream_t stream, const unsigned long long *guards_src) {
    if (pending) return hipSuccess;
    hipError_t e = hipMemcpyAsync(counts, src, n_ * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess && guards_src)
        e = hipMemcpyAsync((void *) guards, guards_src, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipEventRecord(event, stream);
    if (e != hipSuccess) return e;
    pending = true;
    n = n_;
    owner = owner_;
    return hipSuccess;
}
RenderState::Feedback::Landed RenderState::Feedback::take() {
    const bool ready = pending && hipEventQuery(event) == hipSuccess;
    (void) hipGetLastError();      // hipErrorNotReady from the query must not leak into the launch checks that follow
    if (!ready) return {nullptr, 0, kNone};
    pending = false;
    return {counts, n, owner};
}
uint32_t RenderState::Feedback::first_at_most(const uint32_t *counts, uint32_t n, uint32_t threshold) {
    uint32_t k = 0;
    while (k < n && counts[k] > threshold) ++k;
    return k;
}

RenderState::~RenderState() {
    for (void *p : pool) (void) hipFree(p);
    if (host) (void) hipHostFree(host);
    if (event) (void) hipEventDestroy(event);
    if (fb.counts) (void) hipHostFree(fb.counts);
    if (fb.event) (void) hipEventDestroy(fb.event);
    if (last.done) (void) hipEventDestroy(last.done);
    for (hipEvent_t e : timing) (void) hipEventDestroy(e);
    if (counters) (void) hipFree(counters);
    if (aov.rows) (void) hipFree(aov.rows);
    if (sum.limbs) (void) hipFree(sum.limbs);
    for (float *q : conv.scratch)
        if (q) (void) hipFree(q);
    if (conv.ws) (void) hipFree(conv.ws);
    if (conv.ring) (void) hipHostFree(conv.ring);
    for (hipEvent_t e : conv.ev)
        if (e) (void) hipEventDestroy(e);
}

extern "C" {

// ---------------------------------------------------------------------------
// wavefront driver
// ---------------------------------------------------------------------------
static bf_status wf_ensure(const bf_scene *scene, uint32_t capacity) {
    RenderState &run = scene->run;
    bfd::WF &wf = run.wf;
    if (wf.capacity >= capacity) return BF_OK;
    for (void *p : run.pool) (void) hipFree(p);
    run.pool.clear();
    std::memset(&wf, 0, sizeof(wf));
    run.roll_ring = nullptr;
    run.roll_offsets = nullptr;
    auto alloc = [&](void **p, size_t bytes) -> hipError_t {
        hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) run.pool.push_back(*p);
        return e;
    };
    size_t n = capacity, nb = capacity / 64;
    HIP_TRY(alloc((void **) &wf.recA, n * 64));
    HIP_TRY(alloc((void **) &wf.recB, n * 64));
    HIP_TRY(alloc((void **) &wf.recC, n * 64));
    HIP_TRY(alloc((void **) &run.masks, 8 * nb * sizeof(unsigned long long)));
    HIP_TRY(alloc((void **) &wf.n_live, (bfd::kWfMaxIter + 2) * sizeof(uint32_t)));
    HIP_TRY(alloc((void **) &run.roll_ring, bfd::kRollRing * sizeof(bfd::DRoll)));
    HIP_TRY(alloc((void **) &run.roll_offsets, bfd::kRollRing * sizeof(float4)));
    HIP_TRY(alloc((void **) &wf.surv_cursor, 64));
    wf.counters = run.counters;
    wf.capacity = capacity;
    if (!run.host) HIP_TRY(hipHostMalloc((void **) &run.host, 64));
    if (!run.event) HIP_TRY(hipEventCreateWithFlags(&run.event, hipEventDisableTiming));
    if (!run.fb.counts) HIP_TRY(hipHostMalloc((void **) &run.fb.counts, (bfd::kWfMaxIter + 2) * sizeof(uint32_t)));
    if (!run.fb.event) HIP_TRY(hipEventCreateWithFlags(&run.fb.event, hipEventDisableTiming));
    run.fb.guards = reinterpret_cast<volatile unsigned long long *>(run.host) + 1;
    run.plan.valid = false;
    run.fb.drop();
    return BF_OK;
}

// Live slots at which the wavefront iterations hand over to the tail kernel.  A bounce iteration of a nearly empty pool
// costs ~0.5 ms of launch and latency floor whatever it holds, the tail ~25 us per bounce: large pools (the pipelined
// bench step, sweeps) switch at 2^17 live slots — more would keep the tail's 168-VGPR waves on the CUs the next renders'
// kernels want (measured: 2^18 costs 12 % of the pipelined C2 rate) — small pools, whose kernels never fill the chip,
// switch as soon as half the pool is done (C3: 1.21 -> 0.98 ms per render, C4 shard: 1.71 -> 1.30).
static uint32_t wf_tail_threshold(const bf_scene *scene, uint32_t n_slots) {
    if (scene->tun.tail >= 0) return (uint32_t) scene->tun.tail;
    if (n_slots >= bfd::kTailSmallPool) return 1u << 17;
    return std::max<uint32_t>(1u << 17, std::min<uint32_t>(1u << 19, n_slots / 2));
}

namespace {
// Everything the launches of one render (or of one call of a rolling sequence) share.
struct WfCtx {
    const bf_scene *scene;
    const Kernels *k;
    const bfd::DLaunch *lp;
    float *hist;
    bf_path_record *rec;
    hipStream_t stream;
    bool count_nodes, timed;
    size_t mask_bytes, lds_shade, lds_tail;
    unsigned grid_shade, grid_trace;
    unsigned grid_gen[2];   // grids of the launches of wf_shade that start paths ([0] first = 1, [1] the wake launch, first = 2) and
    int gen_waves[2];       // the waves per SIMD they ask for, and
    int gen_build[2];       // the W of the build that request gets (bf_variant.h: shade_variant)
    uint32_t tail_max;
    bool alone;      // nothing else wants the CUs while the tail runs (the flush of a rolling sequence): wf_tail_launch
};

// Dynamic LDS of a launch: [traversal stacks |] histogram, rounded up to 16 bytes | table cache (bf_device_core.h: load_tables_lds).
// wf_shade has no stacks; the tail and the one-kernel variant have.
static_assert(sizeof(int) * bfd::kStackDepth * bfd::kBlock % 16 == 0, "the stacks keep the histogram 16-byte aligned");
constexpr size_t kLdsPerCU = 160u * 1024u;      // gfx950
static size_t lds_bytes(const bfd::DLaunch &lp, uint32_t tab_cache, bool stacks) {
    return (stacks ? sizeof(int) * bfd::kStackDepth * bfd::kBlock : 0u) + ((sizeof(float) * lp.lds_floats + 15) & ~size_t(15)) +
           (tab_cache ? bfd::kTabBytes : 0u);
}
// the histogram of `n_chan` channels is accumulated in LDS
static uint32_t lds_hist(uint32_t n_chan, uint32_t flags) {
    return (n_chan <= (uint32_t) bfd::kMaxLdsHist && !(flags & BF_FLAG_GLOBAL_ATOMICS)) ? 1u : 0u;
}
}  // namespace

// per-kernel timing (stats renders, BF_FLAG_TIMING sequences): one event pair around every launch
static hipError_t wf_tic(const WfCtx &c, int kind) {
    if (!c.timed) return hipSuccess;
    const bf_scene *sc = c.scene;
    while (sc->run.timing.size() < 2 * (sc->run.ev_kind.size() + 1)) {
        hipEvent_t e;
        hipError_t he = hipEventCreate(&e);
        if (he != hipSuccess) return he;
        sc->run.timing.push_back(e);
    }
    sc->run.ev_kind.push_back(kind);
    return hipEventRecord(sc->run.timing[2 * (sc->run.ev_kind.size() - 1)], c.stream);
}
static hipError_t wf_toc(const WfCtx &c) {
    if (!c.timed) return hipSuccess;
    return hipEventRecord(c.scene->run.timing[2 * (c.scene->run.ev_kind.size() - 1) + 1], c.stream);
}
// wait for the stream and add the recorded pairs up by kind (wf_ms), then forget them
static bf_status wf_collect_timing(const bf_scene *scene, hipStream_t stream) {
    scene->run.ms[0] = scene->run.ms[1] = scene->run.ms[2] = 0.f;
    scene->run.tail_launches = scene->run.shade_launches = 0;
    if (scene->run.ev_kind.empty()) return BF_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    for (size_t k = 0; k < scene->run.ev_kind.size(); ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, scene->run.timing[2 * k], scene->run.timing[2 * k + 1]));
        scene->run.ms[scene->run.ev_kind[k]] += ms;
        if (scene->run.ev_kind[k] == 2) ++scene->run.tail_launches;
        if (scene->run.ev_kind[k] == 1) ++scene->run.shade_launches;
    }
    scene->run.ev_kind.clear();
    return BF_OK;
}

// pool size, masks, scheduling knobs and grids for `lp` on this handle
static bf_status wf_setup(const bf_scene *scene, const Kernels &k, const bfd::DLaunch &lp, uint64_t pool_paths, float *hist_dev,
                          bf_path_record *records_dev, hipStream_t stream, bool count_nodes, bool timed, WfCtx &c, bool rolling = false) {
    uint64_t want = std::min<uint64_t>(scene->tun.pool, std::max<uint64_t>(pool_paths, 64));
    uint32_t n_main = (uint32_t) ((want + 63) & ~uint64_t(63)), n_surv = 0;
    if (rolling) {
        // two renders' worth of main slots (a slot's next path is supplied two calls after its current one) + the
        // survivor area for the paths that are still alive by then (bf_wavefront.h)
        n_main = (uint32_t) ((std::max<uint64_t>(2 * pool_paths, 128) + 63) & ~uint64_t(63));
        // at least one survivor batch per shading wave: a wave claims whole batches (surv_claims_max each per launch) and
        // all the claims of one launch must be distinct batches (wf_shade: surv_take)
        const uint32_t surv_min = (uint32_t) scene->n_cus * 4u * (uint32_t) std::max(2, scene->tun.shade_waves) * 64u;
        n_surv = std::max<uint32_t>(surv_min, std::min<uint32_t>(1u << 21, (n_main / 8 + 63) & ~63u));
        // test hook (BF_DEBUG_SURV_BATCHES): a survivor area far too small for the claims its waves may make, to see the loud
        // check of surv_take fire (tests/test_gpu_rolling.py)
        if (scene->tun.debug_surv_batches) n_surv = scene->tun.debug_surv_batches * 64u;
    }
    bf_status st = wf_ensure(scene, n_main + n_surv);
    if (st != BF_OK) return st;
    bfd::WF &wf = scene->run.wf;
    wf.n_main = rolling ? n_main : (uint32_t) ((std::min<uint64_t>(wf.capacity, pool_paths) + 63) & ~uint64_t(63));
    wf.n_surv = n_surv;
    wf.n_slots = wf.n_main + wf.n_surv;
    wf.trace_refill = scene->tun.trace_refill;
    wf.trace_stragglers = scene->tun.trace_stragglers;
    wf.shade_chain = scene->tun.shade_chain;
    wf.row_jobs = scene->tun.row_jobs;
    wf.iq = lp.iq;
    wf.has_render = lp.batch != 0u ? 1u : 0u;
    wf.offsets = lp.batch_offsets;
    wf.has_dop = (lp.doppler || lp.resample) ? 1u : 0u;
    wf.box_slack = lp.box_slack;
    wf.geom_stride = lp.geom_stride;
    const size_t nb = wf.n_slots / 64;
    for (int b = 0; b < 2; ++b) {      // alive | trace | shadow of one parity are contiguous: one memset per bounce
        wf.m_alive[b] = scene->run.masks + (4 * b + 0) * nb;
        wf.m_trace[b] = scene->run.masks + (4 * b + 1) * nb;
        wf.m_shadow[b] = scene->run.masks + (4 * b + 2) * nb;
        wf.m_hit[b] = scene->run.masks + (4 * b + 3) * nb;
    }
    c.scene = scene;
    c.k = &k;
    c.lp = &lp;
    c.hist = hist_dev;
    c.rec = records_dev;
    c.stream = stream;
    c.count_nodes = count_nodes;
    c.timed = timed;
    c.mask_bytes = 4 * nb * sizeof(unsigned long long);
    wf.hit_split = scene->tun.shade_split ? 1u : 0u;
    wf.chain_min = scene->tun.chain_min;
    c.lds_shade = lds_bytes(lp, scene->d.tab_cache, false);
    c.lds_tail = lds_bytes(lp, scene->d.tab_cache, true);
    c.alone = false;
    // persistent grids: shade is register-heavy (its walk: 3 workgroups per CU at 147-153 VGPRs), trace runs
    // 5 workgroups per CU (28.6 KiB of LDS each: stacks + the tree's top levels; 91 VGPRs)
    const unsigned batches_per_block = bfd::kBlock / 64;
    const unsigned max_blocks = (unsigned) ((nb + batches_per_block - 1) / batches_per_block);
    c.grid_shade = std::max(1u, std::min((unsigned) scene->n_cus * (unsigned) std::max(2, scene->tun.shade_waves), max_blocks));
    c.grid_trace = std::max(1u, std::min((unsigned) scene->n_cus * (unsigned) scene->tun.trace_waves, max_blocks));
    // The launches that start paths (first / wake) need fewer registers than the walk: without packed fp32 their four-wave builds are
    // scratch-free (128 VGPRs; profiles/no_slp_resource_usage.txt), so they run four workgroups per CU where such a build exists
    // (bf_variant.h: the W shade_variant answers a request for four with) and four workgroups' dynamic LDS fit a CU; else, and under an
    // explicit BF_SHADE_WAVES, they run as the walk does
    const size_t lds_wg = (c.lds_shade + 16u + 1023u) & ~size_t(1023);      // + wf_shade's static words, in allocation granules (at most 1 KiB)
    for (int first = 1; first <= 2; ++first) {
        const bfv::Shape shape = bfk_launch_shape(lp);
        const bool four = scene->tun.gen_waves == 4 && 4 * lds_wg <= kLdsPerCU && bfv::shade_variant(k.feature, k.fast, shape, first, 4).w == 4;
        c.gen_waves[first - 1] = four ? 4 : scene->tun.shade_waves;
        c.gen_build[first - 1] = bfv::shade_variant(k.feature, k.fast, shape, first, c.gen_waves[first - 1]).w;
        c.grid_gen[first - 1] = four ? std::max(1u, std::min((unsigned) scene->n_cus * 4u, max_blocks)) : c.grid_shade;
    }
    // Small pools never fill the chip: their launches sit at latency floors with nearly idle waves, and a grid sized for the whole GPU
    // keeps the next handle's launch out until it has drained.  Handles that roll side by side (clones of one scene, one per stream)
    // therefore launch a SHARE of the persistent grids each, so that their launches overlap: C3 0.50 -> 0.45 ms per step, a C4 shard
    // 0.62 -> 0.57 with four handles (profiles/r04_grid_share_ab.txt); a handle that rolls alone keeps the full grids (a lone launch
    // is 20 % slower on a third of them).
    if (rolling && scene->tun.grid_share > 1u && wf.n_slots < scene->tun.grid_small) {
        const unsigned peers = (unsigned) std::max(1, scene->peers_rolling->load(std::memory_order_relaxed));
        const unsigned share = std::min(peers, (unsigned) scene->tun.grid_share);
        c.grid_shade = std::max(1u, c.grid_shade / share);
        c.grid_gen[0] = std::max(1u, c.grid_gen[0] / share);
        c.grid_gen[1] = std::max(1u, c.grid_gen[1] / share);
        c.grid_trace = std::max(1u, c.grid_trace / share);
    }
    c.tail_max = wf_tail_threshold(scene, rolling ? wf.n_main / 2 : wf.n_slots);
    wf.surv_claims_max = (wf.n_surv / 64u) / std::max(1u, c.grid_shade * batches_per_block);      // >= 1 by the sizing above
    if (rolling && scene->tun.debug_surv_batches) {                                                   // (the test hook: no rule at all)
        const char *e = getenv("BF_DEBUG_SURV_CLAIMS");
        wf.surv_claims_max = e ? (uint32_t) strtoul(e, nullptr, 10) : 1u << 20;
    }
    return BF_OK;
}
// One bounce iteration `it`: clear the next parity's masks, shade (first: 0 alive masks, 1 first bounce of a pool, 2 alive
// masks then the wake launch of a rolling call), trace.
static bf_status wf_iteration(const WfCtx &c, uint32_t it, int first) {
    const bf_scene *scene = c.scene;
    const bfd::WF &wf = scene->run.wf;
    const int nxt = (it & 1) ^ 1;
    HIP_TRY(hipMemsetAsync(wf.m_alive[nxt], 0, c.mask_bytes, c.stream));     // alive, trace, shadow, hit are contiguous
    if (first != 1) {
        // first launch of a rolling call (first == 2): the evicting variant — long paths make room for the new render's
        HIP_TRY(wf_tic(c, 1));
        HIP_TRY(c.k->shade(&scene->d, c.lp, &wf, it, first == 2 ? 3 : 0, c.hist, c.rec, c.grid_shade, c.lds_shade, c.stream,
                           scene->tun.shade_waves));
        HIP_TRY(wf_toc(c));
    }
    if (first != 0) {
        HIP_TRY(wf_tic(c, 1));
        HIP_TRY(c.k->shade(&scene->d, c.lp, &wf, it, first, c.hist, c.rec, c.grid_gen[first - 1], c.lds_shade, c.stream, c.gen_waves[first - 1]));
        scene->run.gen_waves_last = c.gen_build[first - 1];
        HIP_TRY(wf_toc(c));
    }
    return BF_OK;
}
static bf_status wf_trace_launch(const WfCtx &c, uint32_t it) {
    HIP_TRY(wf_tic(c, 0));
    HIP_TRY(c.k->trace(&c.scene->d, &c.scene->run.wf, it, c.count_nodes ? 1 : 0, c.grid_trace, c.stream, c.scene->tun.trace_waves));
    HIP_TRY(wf_toc(c));
    return BF_OK;
}
static bf_status wf_tail_launch(const WfCtx &c, uint32_t it, uint32_t est_live) {
    const bf_scene *scene = c.scene;
    const bool alone = c.alone;
    // `alone`: nothing else wants the CUs (the flush of a rolling sequence): spread the paths thinly — up to four waves
    // share a batch, so a wave starts with <= 16 paths and walks four lanes per ray from its first bounce instead of
    // waiting for the longest of 64 lane-per-ray walks (half of a tail's cycles are those dense iterations)
    uint32_t share = 1;
    if (!alone && scene->tun.tail_share > 1) {
        share = scene->tun.tail_share >= 4 ? 4u : 2u;
        est_live = (uint32_t) std::min<uint64_t>((uint64_t) est_live * share, 1u << 30);
    }
    if (alone) {
        const uint32_t resident = (uint32_t) scene->n_cus * 4u * 3u;          // waves at 3 per SIMD
        while (share < 4u && (uint64_t) est_live * (share * 2u) / 64u <= resident) share *= 2u;
        est_live = (uint32_t) std::min<uint64_t>((uint64_t) est_live * share, 1u << 30);
    }
    scene->run.wf.tail_share = share;
    HIP_TRY(wf_tic(c, 2));
    HIP_TRY(c.k->tail(&scene->d, c.lp, &scene->run.wf, it, est_live, c.hist, c.rec, c.count_nodes ? 1 : 0, c.lds_tail, c.stream,
                      scene->tun.tail_waves, scene->tun.tail_spread, scene->tun.tail_blocks));
    HIP_TRY(wf_toc(c));
    return BF_OK;
}
// The guard word of wf_trace (CTR_GUARD) is never cleared by a render, so it is sticky across the renders of a handle.
// So is the survivor-area word of rolling sequences (CTR_SURV_GUARD: wf_shade: surv_take refused a claim).
bf_status guard_error(unsigned long long lost, unsigned long long refused) {
    if (lost)
        return fail(BF_ERR_DEVICE, "wf_trace's iteration guard dropped %llu rays in an earlier render of this scene: that render's "
                                   "histogram is wrong (a traversal bug; please report the scene)", lost);
    return fail(BF_ERR_DEVICE, "a launch of a rolling sequence of this scene tried to claim %llu survivor batches beyond the size of "
                               "its survivor area (the claims were refused: no path was lost, but the sizing rule of wf_setup is "
                               "violated; please report the scene and the launch)", refused);
}
// Sticky words found set are reported HERE: clear them (async_on: behind that stream's work; else now, the handle's work has
// completed), drop the copy of them that may be in flight to the next planned render's feedback, and name them.
bf_status report_guards(const bf_scene *scene, unsigned long long lost, unsigned long long refused, const hipStream_t *async_on) {
    unsigned long long *g = scene->run.counters + bfd::CTR_GUARD;
    if (async_on) HIP_TRY(hipMemsetAsync(g, 0, 2 * sizeof(unsigned long long), *async_on));
    else HIP_TRY(hipMemset(g, 0, 2 * sizeof(unsigned long long)));
    scene->run.fb.drop();
    return guard_error(lost, refused);
}
// every path of a completed render / sequence was binned exactly once (CTR_FILM counts film_put calls): the loud form of the
// tests' "sum of the weight channel + invalid samples == paths"
static bf_status check_film_count(const unsigned long long *c, uint64_t n_paths) {
    if (c[bfd::CTR_FILM] != n_paths)
        return fail(BF_ERR_DEVICE, "%llu of %llu paths were binned: paths were lost or binned twice (a scheduling bug; please report the "
                                   "scene and the launch)", (unsigned long long) c[bfd::CTR_FILM], (unsigned long long) n_paths);
    return BF_OK;
}

// The two drive loops of a pool, shared by a stand-alone render and the flush of a rolling sequence.  Per bounce `it`: [zero the
// next masks] -> wf_shade(it) -> wf_trace(it); `it` runs on; first_kind: wf_iteration's `first` of the first iteration.
// Planned: n iterations and the tail, without a host round trip.  The tail kernel finishes whatever is alive, whatever the
// estimate: tail_live (learned) only sizes its grid.
static bf_status drive_planned(const WfCtx &c, uint32_t &it, uint32_t n, int first_kind, uint32_t tail_live) {
    bf_status st;
    for (uint32_t j = 0; j < n; ++j, ++it) {
        if ((st = wf_iteration(c, it, j == 0 ? first_kind : 0)) != BF_OK) return st;
        if ((st = wf_trace_launch(c, it)) != BF_OK) return st;
    }
    return wf_tail_launch(c, it, std::max<uint32_t>(tail_live + tail_live / 4, 64u * bfd::kBlock));
}
// Synchronous: the host reads the live-slot counter of bounce `it` while wf_trace(it) is still running, so the device never idles
// on the decision, and stops after the first bounce that leaves at most c.tail_max slots alive (*n_live of them; the caller
// launches the tail) or after max_iters.
static bf_status drive_sync(const WfCtx &c, uint32_t &it, uint32_t max_iters, int first_kind, uint32_t *n_live) {
    const RenderState &run = c.scene->run;
    volatile uint32_t *hq = run.host;      // [0] = n_live[it]
    bf_status st;
    for (uint32_t j = 0; j < max_iters; ++j) {
        if ((st = wf_iteration(c, it, j == 0 ? first_kind : 0)) != BF_OK) return st;
        HIP_TRY(hipMemcpyAsync((void *) &hq[0], run.wf.n_live + it, sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
        HIP_TRY(hipEventRecord(run.event, c.stream));
        if ((st = wf_trace_launch(c, it)) != BF_OK) return st;
        HIP_TRY(hipEventSynchronize(run.event));
        ++it;
        *n_live = hq[0];
        if (*n_live <= c.tail_max) break;
    }
    return BF_OK;
}

// A stand-alone render.  Its first render of a shape (or any with launch plans off) is driven synchronously and learns how many
// iterations precede the tail; later ones are planned, and the live counts that come back move the switch to where it belongs.
static bf_status aov_attach(const bf_scene *scene, uint64_t slots, bfd::DLaunch &lp);
static bf_status wf_render(const bf_scene *scene, const Kernels &k, const bfd::DLaunch &lp_in, float *hist_dev, bf_path_record *records_dev,
                           hipStream_t stream, bool count_nodes, bool stats, bool aov = false) {
    using Feedback = RenderState::Feedback;
    RenderState &run = scene->run;
    WfCtx c;
    bfd::DLaunch lp = lp_in;      // (the launches read this copy: an AOV render completes it below)
    bf_status st = wf_setup(scene, k, lp, lp.n_paths, hist_dev, records_dev, stream, count_nodes, stats, c);
    if (st != BF_OK) return st;
    bfd::WF &wf = run.wf;
    // BF_FLAG_AOV: one side-row slot per slot of the pool AS SET UP — the pool only grows, and a rolling sequence sizes it beyond
    // tun.pool, so the slots in use are wf_setup's to say, not this launch's
    if (aov && (st = aov_attach(scene, wf.n_slots, lp)) != BF_OK) return st;
    HIP_TRY(hipMemsetAsync(wf.n_live, 0, (bfd::kWfMaxIter + 2) * sizeof(uint32_t), stream));
    run.ev_kind.clear();
    RenderState::Plan &plan = run.plan;
    const Feedback::Landed fb = run.fb.take();
    if (fb.owner == Feedback::kPlan) {      // (counts a rolling call or flush posted are not this plan's: discarded)
        if (run.fb.guards[0] || run.fb.guards[1]) return report_guards(scene, run.fb.guards[0], run.fb.guards[1], &stream);
        const uint32_t at = Feedback::first_at_most(fb.counts, fb.n, plan.tail_max);
        // still above the threshold after the planned iterations: extend
        plan.iters = at < fb.n ? at + 1 : std::min<uint32_t>(fb.n + 2, bfd::kWfMaxIter - 1);
        plan.tail_live = fb.counts[std::min(at, fb.n - 1)];
    }
    uint32_t it = 0;
    if (scene->tun.allow_plan && plan.valid && plan.n_paths == lp.n_paths && plan.mode == lp.mode &&
        plan.max_depth == (uint32_t) lp.max_depth && plan.n_slots == wf.n_slots && plan.tail_max == c.tail_max && plan.iters > 0) {
        if ((st = drive_planned(c, it, plan.iters, 1, plan.tail_live)) != BF_OK) return st;
        HIP_TRY(run.fb.post(wf.n_live, plan.iters, Feedback::kPlan, stream, wf.counters + bfd::CTR_GUARD));
    } else {
        uint32_t n_live = 0;
        if ((st = drive_sync(c, it, bfd::kWfMaxIter, 1, &n_live)) != BF_OK) return st;
        if (n_live > c.tail_max) return fail(BF_ERR_UNSUPPORTED, "path depth exceeded the wavefront iteration limit (%u bounces)", bfd::kWfMaxIter);
        plan = {true, lp.n_paths, lp.mode, (uint32_t) lp.max_depth, wf.n_slots, c.tail_max, it, n_live};
        run.fb.drop();
        if (n_live && (st = wf_tail_launch(c, it, n_live)) != BF_OK) return st;
    }
    run.iters = run.trace_launches = it;
    if (stats) return wf_collect_timing(scene, stream);
    run.ms[0] = run.ms[1] = run.ms[2] = 0.f;
    return BF_OK;
}

// ---------------------------------------------------------------------------
// Rolling sequences (BF_FLAG_ROLLING).  Every render ends in a latency-bound tail of a few long Russian-roulette
// survivors (126-174 bounces among 2^20 paths) that costs a quarter of a 2^24-path step and three quarters of a 2^20-path
// one.  Consecutive renders of one handle that only differ in seed / shard offset / output buffer — the steps of a
// Monte-Carlo accumulation, the pulses of a coherent interval (python_scripts/animated_trans_rad.py:307-384,
// Receive.ipynb cell 30 run such loops one render() / receive() per frame) — therefore form ONE batched launch whose
// path supply grows by one render per call: slot i renders global paths i, i + n_slots, ... (render = g / n_paths), a
// call enqueues a few bounce iterations over the whole pool (first the slots still alive, then a "wake" launch that
// starts the next path of every idle slot), and the survivors of render k simply ride along with the launches of
// renders k + 1, k + 2, ... .  One tail runs per sequence: bf_scene_flush (or anything that needs the pool: another kind
// of render, an endpoint update, a clone).  Every path is the path a stand-alone render would trace (own PCG32 stream).
// ---------------------------------------------------------------------------
static bool roll_same_shape(const bf_launch &a, const bf_launch &b) {
    return a.mode == b.mode && a.color_mode == b.color_mode && a.n_paths == b.n_paths && a.max_depth == b.max_depth &&
           a.rr_depth == b.rr_depth && a.bins == b.bins && a.bins_y == b.bins_y && a.bin_width == b.bin_width &&
           a.time_c == b.time_c && a.flags == b.flags && a.phase_bins == b.phase_bins;
}

// The mesh offsets of a batch's n renders (3 floats each): all finite, *dmax raised to their largest |component|, and *slack = what
// the SHIFT traversal widens a box by (bf_device_core.h: Shift — the roundings of o - d and p + d move a box plane by at most
// 1.8e-7 (S + 2 |d|), S = the bound the boxes were padded for)
static bf_status offsets_slack(const bf_scene *scene, const float *offsets, uint32_t n, const char *who, float *dmax, float *slack) {
    for (uint32_t k = 0; k < n; ++k)
        for (int a = 0; a < 3; ++a) {
            const float q = offsets[3 * k + a];
            if (!std::isfinite(q)) return fail(BF_ERR_INVALID, "%s: non-finite mesh offset of render %u", who, k);
            *dmax = std::max(*dmax, std::fabs(q));
        }
    *slack = 1e-6f * (scene->mesh.origin_scale_built + 2.f * *dmax);
    return BF_OK;
}

// Work of this handle's pool moves from one stream to another: `to` waits (on the device) for what `from` holds so far.
static bf_status hand_over(const bf_scene *scene, hipStream_t from, hipStream_t to) {
    HIP_TRY(hipEventRecord(scene->run.event, from));
    HIP_TRY(hipStreamWaitEvent(to, scene->run.event, 0));
    return BF_OK;
}

// Finish every path of the open sequence: bounce iterations until few slots are alive, then ONE tail launch.  The first
// flush of a sequence shape runs synchronously (the host reads the live count per iteration, as the first render of a
// shape does) and learns how many iterations that takes; later ones enqueue that many without a host round trip.
static bf_status wf_roll_flush(const bf_scene *scene, hipStream_t stream, bool sync_timing) {
    using Feedback = RenderState::Feedback;
    RenderState &run = scene->run;
    RenderState::Roll &r = run.roll;
    if (!r.open) return BF_OK;
    bf_status st;
    if (stream != r.stream && (st = hand_over(scene, r.stream, stream)) != BF_OK) return st;
    bfd::DLaunch &lp = r.lp;
    WfCtx c;
    if ((st = wf_setup(scene, kernels_for(r.shape.flags), lp, (uint64_t) r.per_call * lp.batch_paths, nullptr, nullptr, stream, r.count_nodes, r.timed, c, true)) != BF_OK) return st;
    c.alone = true;
    const Feedback::Landed fb = run.fb.take();
    if (fb.owner == Feedback::kRollFlush) {
        // live counts of the last planned flush: first iteration after which the tail threshold was met
        const uint32_t at = Feedback::first_at_most(fb.counts, fb.n, c.tail_max);
        r.flush_iters = at < fb.n ? at + 1 : std::min<uint32_t>(fb.n + 2, 48u);
        r.flush_live = fb.counts[std::min(at, fb.n - 1)];
    }
    if (r.it + 2u * 64u > bfd::kWfMaxIter) r.it &= 1u;
    const uint32_t it0 = r.it;
    HIP_TRY(hipMemsetAsync(run.wf.n_live + it0, 0, 64 * sizeof(uint32_t), stream));
    if (scene->tun.allow_plan && r.flush_iters > 0) {
        if ((st = drive_planned(c, r.it, r.flush_iters, 0, r.flush_live)) != BF_OK) return st;
        HIP_TRY(run.fb.post(run.wf.n_live + it0, r.it - it0, Feedback::kRollFlush, stream));
    } else {
        uint32_t n_live = 0;
        if ((st = drive_sync(c, r.it, 48u, 0, &n_live)) != BF_OK) return st;
        r.flush_iters = r.it - it0;
        r.flush_live = n_live;
        if (n_live && (st = wf_tail_launch(c, r.it, n_live)) != BF_OK) return st;
    }
    run.iters += r.it - it0;
    run.trace_launches += r.it - it0;
    r.open = false;
    scene->peers_rolling->fetch_sub(1, std::memory_order_relaxed);
    r.multi = false;
    lp.multi = 0u;
    // the sequence's last table version becomes the handle's tables again, behind the flush's kernels
    if ((st = scene->ends.go_home(stream)) != BF_OK) return st;
    if (sync_timing) return wf_collect_timing(scene, stream);
    return BF_OK;
}

static bf_status wf_roll_render(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, const bfd::DLaunch &lp_in,
                                float *hist_dev, bf_path_record *records_dev, hipStream_t stream) {
    RenderState::Roll &r = scene->run.roll;
    bf_status st;
    const uint32_t K = batch ? batch->n_renders : 1u;          // renders this call adds to the sequence
    const bool with_offsets = batch && batch->mesh_offsets && scene->d.n_tris != 0;
    if (r.open && (!roll_same_shape(r.shape, *launch) || r.per_call != K || r.offsets != with_offsets ||
                   r.count + K > bfd::kRollRing || r.stream != stream)) {
        if ((st = wf_roll_flush(scene, r.stream, false)) != BF_OK) return st;
        // the flush ran on the old stream: the new sequence's first launches reuse the pool behind it
        if (r.stream != stream && (st = hand_over(scene, r.stream, stream)) != BF_OK) return st;
    }
    const bool opening = !r.open;
    if (opening) {
        // what the previous sequence of this handle learned (iterations per call, the flush's plan) only fits its shape
        if (!roll_same_shape(r.shape, *launch) || r.per_call != K) r.iters = r.flush_iters = r.flush_live = 0;
        r.shape = *launch;
        r.lp = lp_in;
        r.lp.batch = 1u;
        r.lp.batch_paths = launch->n_paths;
        r.lp.batch_seeds = nullptr;              // seeds, offsets and buffers of a rolling render live in its descriptor
        r.lp.batch_offsets = nullptr;
        r.lp.box_slack = 0.f;
        r.lp.has_records = 0u;
        r.per_call = K;
        r.multi = false;
        r.offsets = with_offsets;
        r.dmax = 0.f;
        r.count = 0;
        r.it = 0;
        r.stream = stream;
        r.count_nodes = (launch->flags & BF_FLAG_STATS) != 0;
        r.timed = (launch->flags & BF_FLAG_TIMING) != 0;
        // LDS window: the newest renders' histogram blocks, as many as fit
        r.window = 1;
        r.lp.lds_hist = lds_hist(lp_in.n_chan, launch->flags);
        if (r.lp.lds_hist) r.window = std::max<uint32_t>(1u, std::min<uint32_t>(bfd::kRollWindow, (uint32_t) bfd::kMaxLdsHist / std::max(1u, lp_in.n_chan)));
        HIP_TRY(hipMemsetAsync(scene->run.counters, 0, sizeof(unsigned long long) * bfd::CTR_GUARD, stream));
        scene->run.ev_kind.clear();
        scene->run.iters = scene->run.trace_launches = 0;
    }
    const bool fresh_pool = opening;
    const uint32_t k = r.count, newest = k + K - 1u;
    bfd::DLaunch &lp = r.lp;
    lp.n_paths = (uint64_t) (k + K) * lp.batch_paths;
    if (r.multi) {                 // the endpoints moved since the sequence was opened: per-path tables from now on (general kernels)
        lp.multi = 1u;
        lp.lean = 0u;
        scene->run.last_variant &= (uint32_t) (BF_VARIANT_FAST | BF_VARIANT_MOMENT);
    }
    lp.roll_newest = newest;
    lp.roll_lo = newest + 1u > r.window ? newest + 1u - r.window : 0u;
    lp.n_chan_all = (lp.roll_newest - lp.roll_lo + 1u) * lp.n_chan;
    lp.base_off = lp.lds_hist ? r.window * lp.n_chan : 0u;        // fixed for the sequence: behind the full window
    lp.lds_floats = lp.base_off + ((r.shape.flags & BF_FLAG_MOMENT) ? bfd::kRollBaseChMoment : bfd::kRollBaseCh) * bfd::kRollBase;
    WfCtx c;
    // slack for the largest offset of the sequence so far (older paths just get wider boxes)
    if (with_offsets && (st = offsets_slack(scene, batch->mesh_offsets, K, "bf_render_batch", &r.dmax, &lp.box_slack)) != BF_OK) return st;
    if ((st = wf_setup(scene, kernels_for(r.shape.flags), lp, (uint64_t) K * lp.batch_paths, nullptr, nullptr, stream, r.count_nodes, r.timed, c, true)) != BF_OK) return st;
    lp.roll = scene->run.roll_ring;           // wf_setup may have (re)allocated the pool and the ring with it
    lp.batch_offsets = with_offsets ? scene->run.roll_offsets : nullptr;
    scene->run.wf.offsets = lp.batch_offsets;
    {
        // the slots due for this call's paths: global paths [k P, (k + K) P) live in slots g mod n_main
        const uint32_t n_main = scene->run.wf.n_main, lo = (uint32_t) (((uint64_t) k * lp.batch_paths) % n_main);
        scene->run.wf.wake_b0 = lo / 64u;
        scene->run.wf.wake_nb = (uint32_t) std::min<uint64_t>(n_main / 64u, ((uint64_t) (lo % 64u) + (uint64_t) K * lp.batch_paths + 63u) / 64u);
    }
    if (fresh_pool) HIP_TRY(hipMemsetAsync(scene->run.wf.surv_cursor, 0, 2 * sizeof(uint32_t), stream));
    const uint32_t n_chan1 = lp.n_chan;
    if (records_dev) lp.has_records = 1u;
    for (uint32_t j = 0; j < K; ++j) {
        bfd::DRoll d;
        d.seed = (batch && batch->seeds) ? batch->seeds[j] : launch->seed;
        d.path_offset = launch->path_offset;
        d.hist = hist_dev + (size_t) j * n_chan1;
        d.records = records_dev ? records_dev + (size_t) j * lp.batch_paths : nullptr;
        d.rects = scene->d.rects;                 // the endpoint tables as they stand for THIS render (kMulti kernels)
        d.shapes = scene->d.shapes;
        d.emitters = scene->d.emitters;
        d.materials = scene->d.materials;
        d.sensor = scene->d.sensor;
        d.c = scene->d.c;
        d.lambda_min = scene->d.lambda_min;
        d.lambda_max = scene->d.lambda_max;
        d.pad = 0u;
        HIP_TRY(bfk_roll_set(scene->run.roll_ring, scene->run.roll_offsets, (k + j) & (bfd::kRollRing - 1u), &d,
                             with_offsets ? batch->mesh_offsets + 3 * j : nullptr, stream));
    }
    // ---- how many bounce iterations this call enqueues ------------------------------------------------
    // A launch that finds fewer live slots than fill the chip a few times over runs at its latency floor whatever it
    // holds, so a call stops iterating once that few are left (roll_live, 1.5 x 2^20 by default: tools/r03_probe9.sh) and leaves them to the next
    // call's launches: too few iterations and too many paths have to move to the survivor area, too many and the late ones
    // run over a nearly empty pool.  Steered by the live counts that come back (without ever waiting for them).
    const RenderState::Feedback::Landed fb = scene->run.fb.take();
    if (fb.owner == RenderState::Feedback::kRollCall && !scene->tun.roll_iters) {
        // round 4: with the shading launches' fixed costs gone (the statistics atomics) a launch over a FULL pool is what
        // pays: a call of a big render stops after its first iteration as long as at most a quarter of the main slots
        // is alive (C2 / C5: one iteration per call instead of three: wf_trace 3.80 -> 3.27 ms per step, profiles/
        // r04_roll_iterations.txt); what is still alive two calls later moves to the survivor area as before
        const uint32_t live_max = scene->tun.roll_live ? scene->tun.roll_live : std::max<uint32_t>(3u << 19, scene->run.wf.n_main / 4u);
        r.iters = std::min<uint32_t>(RenderState::Feedback::first_at_most(fb.counts, fb.n, live_max) + 1u, 16u);
    }
    if (scene->tun.roll_iters) r.iters = scene->tun.roll_iters;
    if (r.iters == 0) r.iters = 2;
    if (r.it + 2u * 64u > bfd::kWfMaxIter) r.it &= 1u;       // the live-counter ring: keep the parity, restart the index
    const uint32_t it0 = r.it, I = r.iters;
    HIP_TRY(hipMemsetAsync(scene->run.wf.n_live + it0, 0, I * sizeof(uint32_t), stream));
    for (uint32_t j = 0; j < I; ++j) {
        const uint32_t it = r.it;
        if ((st = wf_iteration(c, it, j == 0 ? (opening ? 1 : 2) : 0)) != BF_OK) return st;
        if ((st = wf_trace_launch(c, it)) != BF_OK) return st;
        ++r.it;
    }
    scene->run.iters += I;
    scene->run.trace_launches += I;
    HIP_TRY(scene->run.fb.post(scene->run.wf.n_live + it0, I, RenderState::Feedback::kRollCall, stream));
    if (!r.open) scene->peers_rolling->fetch_add(1, std::memory_order_relaxed);
    r.open = true;
    r.count += K;
    return BF_OK;
}

// counters -> bf_stats (+ the per-kernel times of the last timed render / sequence)
void fill_stats(const bf_scene *scene, const unsigned long long *c, uint64_t n_paths, bf_stats *st) {
    std::memset(st, 0, sizeof(*st));
    st->n_paths = n_paths;
    st->n_rays_closest = c[bfd::CTR_CLOSEST];
    st->n_rays_shadow = c[bfd::CTR_SHADOW];
    st->n_nodes_visited = c[bfd::CTR_NODES];
    st->n_nodes_lds = c[bfd::CTR_NODES_LDS];
    st->n_tris_tested = c[bfd::CTR_TRIS];
    st->n_invalid = c[bfd::CTR_INVALID];
    st->n_bounces = c[bfd::CTR_BOUNCES];
    st->n_rays_tail = c[bfd::CTR_TAIL_RAYS];
    st->n_rays_traced = c[bfd::CTR_TRACED];
    st->n_nodes_tail = c[bfd::CTR_TAIL_NODES];
    st->n_wnodes_tail = c[bfd::CTR_TAIL_WNODES];
    st->n_tris_tail = c[bfd::CTR_TAIL_TRIS];
    st->n_bounces_tail = c[bfd::CTR_TAIL_BOUNCES];
    st->n_shade_loads = c[bfd::CTR_SHADE_LOADS];
    st->n_shade_stores = c[bfd::CTR_SHADE_STORES];
    st->n_shade_shadow = c[bfd::CTR_SHADE_SHADOW];
    st->n_shade_rays = c[bfd::CTR_SHADE_RAYS];
    st->n_guard = c[bfd::CTR_GUARD];
    st->trace_ms = scene->run.ms[0];
    st->shade_ms = scene->run.ms[1];
    st->tail_ms = scene->run.ms[2];
    st->n_launches_trace = scene->run.trace_launches;
    st->n_bounce_iters = scene->run.iters;
    st->n_launches_tail = scene->run.tail_launches;
    st->n_launches_shade = scene->run.shade_launches;
    st->kernel_variant = scene->run.last_variant;
}

void add_stats(bf_stats &a, const bf_stats &b) {
    a.n_paths += b.n_paths;
    a.n_rays_closest += b.n_rays_closest;
    a.n_rays_shadow += b.n_rays_shadow;
    a.n_nodes_visited += b.n_nodes_visited;
    a.n_tris_tested += b.n_tris_tested;
    a.n_invalid += b.n_invalid;
    a.n_bounces += b.n_bounces;
    a.kernel_ms += b.kernel_ms;
    a.trace_ms += b.trace_ms;
    a.shade_ms += b.shade_ms;
    a.tail_ms += b.tail_ms;
    a.n_launches_trace += b.n_launches_trace;
    a.n_bounce_iters += b.n_bounce_iters;
    a.n_rays_tail += b.n_rays_tail;
    a.n_rays_traced += b.n_rays_traced;
    a.n_nodes_lds += b.n_nodes_lds;
    a.n_nodes_tail += b.n_nodes_tail;
    a.n_wnodes_tail += b.n_wnodes_tail;
    a.n_tris_tail += b.n_tris_tail;
    a.n_bounces_tail += b.n_bounces_tail;
    a.n_shade_loads += b.n_shade_loads;
    a.n_shade_stores += b.n_shade_stores;
    a.n_shade_shadow += b.n_shade_shadow;
    a.n_shade_rays += b.n_shade_rays;
    a.n_guard += b.n_guard;
    a.kernel_variant |= b.kernel_variant;      // (the chunks of a batch, the rounds of a converge call, run the same kernels)
}

// Stream order between the successive uses of a handle's pool: work enqueued on another stream than the previous
// call's waits for it (an event wait on the device, never on the host).
bf_status order_after_last(const bf_scene *scene, hipStream_t stream) {
    const RenderState::LastUse &last = scene->run.last;
    if (last.has && last.stream != stream) HIP_TRY(hipStreamWaitEvent(stream, last.done, 0));
    return BF_OK;
}
bf_status mark_last(const bf_scene *scene, hipStream_t stream) {
    RenderState::LastUse &last = scene->run.last;
    if (!last.done) HIP_TRY(hipEventCreateWithFlags(&last.done, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(last.done, stream));
    last.stream = stream;
    last.has = true;
    return BF_OK;
}
// anything but another render of the open rolling sequence needs the pool (or the scene tables) to itself
bf_status close_sequence(const bf_scene *scene, hipStream_t stream) {
    if (!scene->run.roll.open) return BF_OK;
    bf_status st = wf_roll_flush(scene, stream, false);
    if (st != BF_OK) return st;
    return mark_last(scene, stream);
}

// The statistics of the handle's completed work: counters -> stats_out, kernel_ms from the event pair around it (destroyed here) or,
// without one, the per-kernel times; then the sticky guard words, then (check_film) that every path was binned.
static bf_status read_stats(const bf_scene *scene, uint64_t n_paths, bf_stats *stats_out, bool check_film, hipEvent_t ev0 = nullptr,
                            hipEvent_t ev1 = nullptr) {
    unsigned long long c[bfd::CTR_COUNT];
    HIP_TRY(hipMemcpy(c, scene->run.counters, sizeof(c), hipMemcpyDeviceToHost));
    fill_stats(scene, c, n_paths, stats_out);
    stats_out->kernel_ms = scene->run.ms[0] + scene->run.ms[1] + scene->run.ms[2];
    if (ev0) {
        const hipError_t he = hipEventElapsedTime(&stats_out->kernel_ms, ev0, ev1);
        (void) hipEventDestroy(ev0);
        (void) hipEventDestroy(ev1);
        if (he != hipSuccess) return fail(BF_ERR_DEVICE, "hipEventElapsedTime: %s", hipGetErrorString(he));
    }
    if (c[bfd::CTR_GUARD] || c[bfd::CTR_SURV_GUARD]) return report_guards(scene, c[bfd::CTR_GUARD], c[bfd::CTR_SURV_GUARD]);
    return check_film ? check_film_count(c, n_paths) : BF_OK;
}

// The lean profile (bf_device.h: kLean): what the scene and the launch must look like for the kernels that have everything else
// compiled out.  Every radar scene of the reference's scripts and every BASELINE config fits; anything else runs the
// general kernels (same results: tests/test_gpu_parity.py::test_lean_and_general_kernels_agree).
static bool lean_profile(const bf_scene *scene, const bf_launch *launch, bool receive_mode, bool multi_pixel) {
    const EndpointState &ends = scene->ends;
    // lean builds exist of the default register budgets only (the walk launches and the tail at three waves per SIMD; the generation
    // launches' budget, tun.gen_waves, is not a condition: they have lean builds at three and at four), and not of the one-kernel variant
    if ((launch->flags & BF_FLAG_MEGAKERNEL) || scene->tun.shade_waves != 3 || scene->tun.tail_waves != 3) return false;
    if (!scene->tun.lean || scene->d.n_emitters != 1 || scene->d.uvs != nullptr || ends.sensor_host.filt_n != 0u) return false;
    if (ends.sensor_host.win_off_t || ends.sensor_host.win_off_f) return false;      // ADC window away from the origin
    if (ends.sensor_host.crop_x || ends.sensor_host.crop_y) return false;            // film crop window away from the origin
    if (ends.any_back_material) return false;                                        // twosided with two nested BSDFs
    if (ends.any_resample) return false;                                             // resample_freq transmitters
    const uint32_t et = ends.emitter_types[0];
    if (receive_mode)
        return (et == BF_TRANSMITTER_AREA || et == BF_TRANSMITTER_WIGNER) && ends.sensor_host.type == BF_RECEIVER_OMNI &&
               launch->phase_bins == 0 && !(launch->flags & (BF_FLAG_DOPPLER | BF_FLAG_MIX_RESAMPLE));
    return et == BF_EMITTER_AREA && ends.sensor_host.type == BF_SENSOR_PERSPECTIVE && !multi_pixel && launch->mode != BF_MODE_TIME;
}

static bool receive_mode_of(const bf_launch *launch) { return launch->mode == BF_MODE_RECEIVE_RAW || launch->mode == BF_MODE_RECEIVE_IQ; }
static bool multi_pixel_of(const bf_launch *launch) { return launch->spp && launch->film_width && launch->film_height; }

// What a BF_FLAG_CLASSES launch (of n_renders renders) is refused for; the motion / deform batches ask before they enqueue their
// geometry versions, every launch asks again in check_launch
bf_status check_classes(const bf_scene *scene, const bf_launch *launch, uint32_t n_renders) {
    if (launch->flags & BF_FLAG_CLASSES) {
        const uint32_t n_classes = bfd::scene_n_classes(scene->d);
        if (!n_classes) return fail(BF_ERR_INVALID, "BF_FLAG_CLASSES: the scene has no class table (bf_scene_set_classes)");
        if (launch->flags & (BF_FLAG_FAST | BF_FLAG_MOMENT))
            return fail(BF_ERR_INVALID, "BF_FLAG_CLASSES with %s: the class variants exist of the exact first-moment kernels only",
                        (launch->flags & BF_FLAG_FAST) ? "BF_FLAG_FAST" : "BF_FLAG_MOMENT");
        if (launch->flags & BF_FLAG_ROLLING)
            return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_CLASSES with BF_FLAG_ROLLING: a rolling sequence's histogram window and base-channel "
                                            "table hold one block per render; render the classes without BF_FLAG_ROLLING");
        if ((uint64_t) n_renders * n_classes * bf_launch_channels(launch) > (1ull << 31))
            return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_CLASSES: %u renders x %u classes x %u channels is too large", n_renders, n_classes,
                        bf_launch_channels(launch));
    }
    return BF_OK;
}

// What a BF_FLAG_AOV launch is refused for; asked where check_classes is
bf_status check_aov(const bf_scene *scene, const bf_launch *launch, uint32_t n_renders) {
    if (!(launch->flags & BF_FLAG_AOV)) return BF_OK;
    if (!scene->run.aov.n) return fail(BF_ERR_INVALID, "BF_FLAG_AOV: the scene has no AOV table (bf_scene_set_aovs)");
    if (launch->mode == BF_MODE_RECEIVE_RAW || launch->mode == BF_MODE_RECEIVE_IQ)
        return fail(BF_ERR_INVALID, "BF_FLAG_AOV in a receive mode: the aov integrator wraps a sampling integrator and writes a film; the ADC has no AOV channels");
    if (launch->flags & (BF_FLAG_FAST | BF_FLAG_MOMENT | BF_FLAG_CLASSES))
        return fail(BF_ERR_INVALID, "BF_FLAG_AOV with %s: the AOV variants exist of the exact first-moment kernels only",
                    (launch->flags & BF_FLAG_FAST) ? "BF_FLAG_FAST" : ((launch->flags & BF_FLAG_MOMENT) ? "BF_FLAG_MOMENT" : "BF_FLAG_CLASSES"));
    if (launch->flags & BF_FLAG_ROLLING)
        return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_AOV with BF_FLAG_ROLLING: a rolling sequence's histogram window and base-channel table are "
                                        "laid out for the plain channels; render the AOVs without BF_FLAG_ROLLING");
    const uint64_t px = multi_pixel_of(launch) ? (uint64_t) launch->film_width * launch->film_height : 1u;
    const uint32_t K = bf_aov_floats(scene->run.aov.n, scene->run.aov.types);
    if ((uint64_t) n_renders * (bf_launch_channels(launch) + px * (K + 4u)) > (1ull << 31))
        return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_AOV: %u renders x %llu pixels x %u AOV floats is too large", n_renders, (unsigned long long) px, K);
    return BF_OK;
}

// What a BF_FLAG_EXACT_SUM launch is refused for; asked where check_classes is
bf_status check_sum(const bf_scene *scene, const bf_launch *launch, uint32_t n_renders) {
    (void) scene;
    (void) n_renders;
    if (!(launch->flags & BF_FLAG_EXACT_SUM)) return BF_OK;
    if (launch->flags & (BF_FLAG_FAST | BF_FLAG_MOMENT | BF_FLAG_CLASSES | BF_FLAG_AOV))
        return fail(BF_ERR_INVALID, "BF_FLAG_EXACT_SUM with %s: the exact-sum variants exist of the exact first-moment kernels only",
                    (launch->flags & BF_FLAG_FAST) ? "BF_FLAG_FAST"
                                                   : ((launch->flags & BF_FLAG_MOMENT) ? "BF_FLAG_MOMENT" : ((launch->flags & BF_FLAG_CLASSES) ? "BF_FLAG_CLASSES" : "BF_FLAG_AOV")));
    if (launch->flags & BF_FLAG_ROLLING)
        return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_EXACT_SUM with BF_FLAG_ROLLING: the LDS window of a rolling sequence is laid out in floats; "
                                        "render exact sums without BF_FLAG_ROLLING");
    // a cell takes at most one addend per path of its render, and a limb holds the pieces of fewer than 2^31 addends (bf_sum.h)
    if (launch->n_paths >= bfs::kMaxAddends)
        return fail(BF_ERR_INVALID, "BF_FLAG_EXACT_SUM: n_paths %llu is not below 2^31, the addends a cell is exact for", (unsigned long long) launch->n_paths);
    return BF_OK;
}

// Everything a launch (of n_renders renders, if a batch) is refused for on its own or against the scene and its open rolling sequence:
// nothing is enqueued before these
static bf_status check_launch(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, uint32_t n_renders, const bf_stats *stats_out) {
    const EndpointState &ends = scene->ends;
    if (bf_status sst = check_sum(scene, launch, n_renders)) return sst;
    if (bf_status cst = check_classes(scene, launch, n_renders)) return cst;
    if (bf_status ast = check_aov(scene, launch, n_renders)) return ast;
    if (batch) {
        if (n_renders == 0) return fail(BF_ERR_INVALID, "bf_render_batch: n_renders is 0");
        if (launch->spp && launch->film_width && launch->film_height)
            return fail(BF_ERR_UNSUPPORTED, "bf_render_batch: multi-pixel films are rendered one launch at a time");
        if ((uint64_t) n_renders * bf_launch_channels(launch) > (1ull << 31) || (uint64_t) n_renders * launch->n_paths >= (1ull << 48))
            return fail(BF_ERR_UNSUPPORTED, "bf_render_batch: %u renders x %llu paths is too large", n_renders, (unsigned long long) launch->n_paths);
    }
    const bool is_rx = ends.sensor_host.type == BF_RECEIVER_OMNI || ends.sensor_host.type == BF_RECEIVER_WIGNER ||
                       ends.sensor_host.type == BF_RECEIVER_PHASED;
    const bool receive_mode = receive_mode_of(launch);
    if (receive_mode) {
        if (!is_rx) return fail(BF_ERR_INVALID, "receive mode needs a receiver (omnidirectional / wigner)");
        if (launch->bins != ends.adc_t || launch->bins_y != ends.adc_f)
            return fail(BF_ERR_INVALID, "receive mode: launch bins (%u x %u) must equal the ADC size — its window, if it has one — (%u x %u)",
                        launch->bins, launch->bins_y, ends.adc_t, ends.adc_f);
        for (uint32_t i = 0; i < scene->d.n_emitters; ++i)
            if (ends.emitter_types[i] != BF_TRANSMITTER_AREA && ends.emitter_types[i] != BF_TRANSMITTER_WIGNER &&
                ends.emitter_types[i] != BF_TRANSMITTER_PHASED)
                return fail(BF_ERR_INVALID, "receive mode: emitter %u is not a transmitter", i);
        // the Wigner and phased receivers sample their own local-oscillator signal under "mix_resample" (wignerreceiver.cpp:72-110,
        // 172-189): a delta signal's instantaneous frequency at the receive time (sample_delta_frequency :149-166: a chirp's or a
        // carrier's; "pulse" leaves it uninitialised there: refused), or a uniform frequency weighted with eval_signal
        if ((launch->flags & BF_FLAG_MIX_RESAMPLE) && ends.sensor_host.type != BF_RECEIVER_OMNI) {
            if (ends.sensor_host.rx_sig_is_delta && ends.sensor_host.rx_signal == BF_SIGNAL_PULSE)
                return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_MIX_RESAMPLE on the Wigner / phased receiver: a \"pulse\" local oscillator that is a delta "
                                                "signal reads an uninitialised frequency in the reference (wignerreceiver.cpp:149-166)");
            if (ends.sensor_host.rx_signal != BF_SIGNAL_CW && !(ends.sensor_host.rx_pulse_len > 0.f && ends.sensor_host.rx_prf > 0.f))
                return fail(BF_ERR_INVALID, "BF_FLAG_MIX_RESAMPLE: the receiver's chirp / pulse needs rx_pulse_len > 0 and rx_prf > 0");
        }
    } else {
        if (launch->flags & BF_FLAG_MIX_RESAMPLE) return fail(BF_ERR_INVALID, "BF_FLAG_MIX_RESAMPLE is a receive-mode flag");
        if (is_rx) return fail(BF_ERR_INVALID, "render modes need a sensor (fluxmeter / perspective), not a receiver");
        for (uint32_t i = 0; i < scene->d.n_emitters; ++i)
            if (ends.emitter_types[i] != BF_EMITTER_SPOT && ends.emitter_types[i] != BF_EMITTER_AREA &&
                ends.emitter_types[i] != BF_EMITTER_POINT)
                return fail(BF_ERR_INVALID, "render modes: emitter %u is a transmitter (use receive mode)", i);
    }
    if (launch->mode > BF_MODE_RECEIVE_IQ) return fail(BF_ERR_INVALID, "unknown mode %u", launch->mode);
    if (launch->mode != BF_MODE_RECEIVE_RAW && launch->phase_bins)
        return fail(BF_ERR_INVALID, "phase_bins needs receive mode (PhaseIntegrator wraps pathtimefrequency)");
    if (launch->phase_bins > 4096) return fail(BF_ERR_INVALID, "phase_bins %u out of range", launch->phase_bins);
    if ((launch->mode == BF_MODE_RANGE || launch->mode == BF_MODE_TIME) && (launch->bins == 0 || !(launch->bin_width > 0.f)))
        return fail(BF_ERR_INVALID, "range/time mode needs bins > 0 and bin_width > 0");
    const bool multi_pixel = multi_pixel_of(launch);
    if (multi_pixel ? (launch->film_width != ends.film_w || launch->film_height != ends.film_h)
                    : (ends.film_w != 1 || ends.film_h != 1) && !is_rx)
        return fail(BF_ERR_INVALID, "the sensor's film is %u x %u: the launch must name the same film and spp > 0 (it has %u x %u, spp %u)",
                    ends.film_w, ends.film_h, launch->film_width, launch->film_height, launch->spp);
    if (multi_pixel) {
        if (launch->mode == BF_MODE_RECEIVE_RAW || launch->mode == BF_MODE_RECEIVE_IQ)
            return fail(BF_ERR_INVALID, "receive modes bin into the ADC: film_width / film_height / spp must be 0");
        const uint64_t px = (uint64_t) launch->film_width * launch->film_height;
        if (px > (1u << 24) || px * (5ull + 3ull * launch->bins) > (1ull << 31))
            return fail(BF_ERR_UNSUPPORTED, "film %u x %u with %u bins is too large", launch->film_width, launch->film_height, launch->bins);
        if (launch->path_offset + launch->n_paths > px * launch->spp)
            return fail(BF_ERR_INVALID, "path_offset + n_paths = %llu exceeds film_width * film_height * spp = %llu",
                        (unsigned long long) (launch->path_offset + launch->n_paths), (unsigned long long) (px * launch->spp));
    }
    if ((launch->flags & BF_FLAG_MOMENT) && (launch->flags & BF_FLAG_FAST))
        return fail(BF_ERR_INVALID, "BF_FLAG_MOMENT | BF_FLAG_FAST: the fast-arithmetic tolerance contract says nothing about squared "
                                    "samples; render second moments with the exact kernels");
    if (multi_pixel && (launch->flags & BF_FLAG_MOMENT) && (uint64_t) launch->film_width * launch->film_height * (11ull + 6ull * launch->bins) > (1ull << 31))
        return fail(BF_ERR_UNSUPPORTED, "film %u x %u with %u bins and BF_FLAG_MOMENT is too large", launch->film_width, launch->film_height, launch->bins);
    if (launch->flags & BF_FLAG_ROLLING) {
        // one sequence, one arithmetic: its long paths are finished by the kernels of the mode it was opened with
        if (scene->run.roll.open && ((launch->flags ^ scene->run.roll.shape.flags) & BF_FLAG_FAST))
            return fail(BF_ERR_INVALID, "BF_FLAG_ROLLING: the open rolling sequence of this handle was started %s BF_FLAG_FAST; "
                                        "flush it (bf_scene_flush) before rolling renders of the other mode",
                        (scene->run.roll.shape.flags & BF_FLAG_FAST) ? "with" : "without");
        // ... and one channel layout: its histograms' base-channel table has five or eleven entries per render
        if (scene->run.roll.open && ((launch->flags ^ scene->run.roll.shape.flags) & BF_FLAG_MOMENT))
            return fail(BF_ERR_INVALID, "BF_FLAG_ROLLING: the open rolling sequence of this handle was started %s BF_FLAG_MOMENT; "
                                        "flush it (bf_scene_flush) before rolling renders of the other layout",
                        (scene->run.roll.shape.flags & BF_FLAG_MOMENT) ? "with" : "without");
        if (multi_pixel || (launch->flags & BF_FLAG_MEGAKERNEL))
            return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_ROLLING: multi-pixel films and the one-kernel variant do not roll");
        if (stats_out)
            return fail(BF_ERR_INVALID, "BF_FLAG_ROLLING: a rolling render returns before its paths have ended, so it has no statistics "
                                        "of its own (pass stats_out = NULL; bf_scene_flush reports the sequence's)");
    }
    return BF_OK;
}

// The device launch of `launch` (x n_renders) on this scene, and the handle's kernel variant with it.  `count`: the kernels count
// rays and film writes.
static bf_status make_dlaunch(const bf_scene *scene, const bf_launch *launch, uint32_t n_renders, uint32_t geom_stride, bool count, bfd::DLaunch &lp) {
    const bool receive_mode = receive_mode_of(launch), multi_pixel = multi_pixel_of(launch);
    std::memset(&lp, 0, sizeof(lp));
    lp.film_w = multi_pixel ? launch->film_width : 1u;
    lp.film_h = multi_pixel ? launch->film_height : 1u;
    lp.spp = multi_pixel ? launch->spp : 0u;
    lp.mode = launch->mode;
    lp.color_mode = launch->color_mode;
    lp.n_paths = launch->n_paths;
    lp.path_offset = launch->path_offset;
    lp.seed = launch->seed;
    lp.max_depth = launch->max_depth;
    lp.rr_depth = launch->rr_depth;
    lp.bins = launch->bins;
    lp.bins_y = launch->bins_y;
    lp.phase_bins = launch->mode == BF_MODE_RECEIVE_RAW ? launch->phase_bins : 0u;
    lp.iq = launch->mode == BF_MODE_RECEIVE_IQ ? 1u : 0u;
    if (lp.iq) lp.mode = BF_MODE_RECEIVE_RAW;          // the kernels see receive mode + the iq flag
    lp.bin_width = launch->bin_width;
    lp.time_c = launch->time_c;
    lp.n_chan = (launch->flags & BF_FLAG_AOV) ? bf_scene_launch_channels(scene, launch) : bf_launch_channels(launch);
    lp.chan_px = lp.n_chan / (lp.film_w * lp.film_h);
    lp.lean = lean_profile(scene, launch, receive_mode, multi_pixel) ? 1u : 0u;
    lp.wide = scene->ends.sensor_host.filt_n != 0u ? 1u : 0u;
    // (wide: reconstruction filter wider than a pixel: the kernels' kWide variants)
    scene->run.last_variant = (lp.lean ? (uint32_t) BF_VARIANT_LEAN : 0u) | (lp.wide ? (uint32_t) BF_VARIANT_WIDE : 0u);
    if (launch->flags & BF_FLAG_FAST) scene->run.last_variant |= (uint32_t) BF_VARIANT_FAST;
    if (launch->flags & BF_FLAG_MOMENT) scene->run.last_variant |= (uint32_t) BF_VARIANT_MOMENT;
    // the class variants exist of the general forms only: a lean scene runs them too, and says so
    const uint32_t n_classes = (launch->flags & BF_FLAG_CLASSES) ? bfd::scene_n_classes(scene->d) : 0u;
    if (n_classes) {
        lp.lean = 0u;
        scene->run.last_variant = (scene->run.last_variant & ~(uint32_t) BF_VARIANT_LEAN) | (uint32_t) BF_VARIANT_CLASS;
    }
    if (launch->flags & BF_FLAG_AOV) {      // likewise; the table and the side rows join the launch in render_locked (aov_attach)
        lp.lean = 0u;
        scene->run.last_variant = (scene->run.last_variant & ~(uint32_t) BF_VARIANT_LEAN) | (uint32_t) BF_VARIANT_AOV;
    }
    const bool exact_sum = (launch->flags & BF_FLAG_EXACT_SUM) != 0u;
    if (exact_sum) {                        // likewise; the limb cells join the launch in render_locked (sum_attach)
        lp.lean = 0u;
        scene->run.last_variant = (scene->run.last_variant & ~(uint32_t) BF_VARIANT_LEAN) | (uint32_t) BF_VARIANT_EXACT_SUM;
    }
    lp.count = ((launch->flags & (BF_FLAG_STATS | BF_FLAG_COUNT)) || count) ? 1u : 0u;
    lp.doppler = (receive_mode && (launch->flags & BF_FLAG_DOPPLER)) ? 1u : 0u;
    lp.resample = (receive_mode && scene->ends.any_resample) ? 1u : 0u;
    if (lp.resample && lp.doppler)
        return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_DOPPLER with a resample_freq transmitter: both rewrite the path's wavelength (one slot of path state)");
    lp.mix = (receive_mode && (launch->flags & BF_FLAG_MIX_RESAMPLE)) ? 1u : 0u;
    lp.n_chan_all = lp.n_chan * n_renders * std::max(1u, n_classes);      // [render][class][n_chan]: LDS privatisation is decided on all of it
    lp.geom_stride = geom_stride;
    lp.lds_hist = lds_hist(lp.n_chan_all, launch->flags);
    lp.lds_floats = lp.lds_hist ? lp.n_chan_all : 0u;
    // a class launch of a 1 x 1 film that cannot privatise its histogram still sums the five base channels of every class block per
    // workgroup: without that every path of the launch adds to the same 5 n_classes global addresses (tools/class_ab.py: C4)
    if (n_classes && !lp.lds_hist && !receive_mode && !multi_pixel && (uint64_t) n_renders * n_classes * bfd::kRollBaseCh <= (uint64_t) bfd::kMaxLdsHist)
        lp.lds_floats = n_renders * n_classes * bfd::kRollBaseCh;
    if (exact_sum) {
        // limb cells of bfs::kCellFloats floats each (bf_sum.h): privatised when n_chan_all of them fit what kMaxLdsHist stands for; a
        // 1 x 1 film that cannot still sums its five base channels per workgroup, in a table [render][5] of cells: without that every
        // path of the launch adds to the same five global cells (the class precedent above)
        const uint64_t cell_floats = (uint64_t) bfs::kCellFloats;
        lp.lds_hist = ((uint64_t) lp.n_chan_all * cell_floats <= (uint64_t) bfd::kMaxLdsHist && !(launch->flags & BF_FLAG_GLOBAL_ATOMICS)) ? 1u : 0u;
        lp.lds_floats = lp.lds_hist ? lp.n_chan_all * (uint32_t) cell_floats : 0u;
        if (!lp.lds_hist && !receive_mode && !multi_pixel && (uint64_t) n_renders * bfd::kRollBaseCh * cell_floats <= (uint64_t) bfd::kMaxLdsHist)
            lp.lds_floats = n_renders * bfd::kRollBaseCh * (uint32_t) cell_floats;
    }
    return BF_OK;
}

// A batch that does not roll is one launch sequence over n_renders * n_paths global path indices (DLaunch::batch); the per-render
// seeds and mesh offsets travel through the scene's pinned staging ring, so the caller's arrays are free on return
static bf_status stage_batch(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, hipStream_t stream, bfd::DLaunch &lp) {
    const uint32_t n_renders = batch->n_renders;
    lp.batch = n_renders;
    lp.batch_paths = launch->n_paths;
    lp.n_paths = launch->n_paths * n_renders;
    // the offsets are read as float4 on both sides: keep them 16-byte aligned behind the seeds
    const size_t seed_bytes = batch->seeds ? ((sizeof(uint64_t) * n_renders + 15) & ~size_t(15)) : 0;
    const size_t off_bytes = batch->mesh_offsets ? sizeof(float4) * n_renders : 0;
    if (!(seed_bytes + off_bytes)) return BF_OK;
    bf_scene::Stage *stg = nullptr;
    bf_status st = stage_acquire(scene, seed_bytes + off_bytes, &stg);
    if (st != BF_OK) return st;
    if (seed_bytes) {
        std::memcpy(stg->host, batch->seeds, sizeof(uint64_t) * n_renders);
        lp.batch_seeds = (const uint64_t *) stg->dev;
    }
    if (off_bytes) {
        float dmax = 0.f, slack = 0.f;
        if ((st = offsets_slack(scene, batch->mesh_offsets, n_renders, "bf_render_batch", &dmax, &slack)) != BF_OK) return st;
        float4 *o = (float4 *) ((char *) stg->host + seed_bytes);
        for (uint32_t k = 0; k < n_renders; ++k) o[k] = make_float4(batch->mesh_offsets[3 * k], batch->mesh_offsets[3 * k + 1], batch->mesh_offsets[3 * k + 2], 0.f);
        if (scene->d.n_tris) {
            lp.batch_offsets = (const float4 *) ((char *) stg->dev + seed_bytes);
            lp.box_slack = slack;
        }
    }
    return stage_commit(stg, seed_bytes + off_bytes, stream);
}

// BF_FLAG_AOV: the handle's table and side rows for `slots` slots into the launch's five words (bf_device.h: AovCtx).  The rows are the
// handle's own, grown on demand; the renders of one handle are ordered on the device (order_after_last), so one set serves them all.
static bf_status aov_attach(const bf_scene *scene, uint64_t slots, bfd::DLaunch &lp) {
    // (called after wf_setup / with the one-kernel variant's grid: `slots` is what the kernels index the rows with, exactly)
    RenderState::Aov &a = scene->run.aov;
    uint64_t types = 0;
    uint32_t mask = 0, rows = 0;
    for (uint32_t i = 0; i < a.n; ++i) {
        types |= (uint64_t) (a.types[i] + 1u) << (4u * i);
        if (a.types[i] < bfd::kAovStored && !(mask >> a.types[i] & 1u)) {
            mask |= 1u << a.types[i];
            rows += bfd::aov_type_floats(a.types[i]);
        }
    }
    if (slots >= (1ull << 32)) return fail(BF_ERR_UNSUPPORTED, "BF_FLAG_AOV: %llu path slots", (unsigned long long) slots);
    const uint64_t need = std::max<uint64_t>(1, (uint64_t) rows * slots);
    if (a.rows_floats < need) {
        if (a.rows) {
            // as wf_ensure grows the pool: hipFree waits for the device, so an earlier launch that reads the old rows has ended
            (void) hipFree(a.rows);
            a.rows = nullptr;
            a.rows_floats = 0;
        }
        HIP_TRY(hipMalloc((void **) &a.rows, need * sizeof(float)));
        a.rows_floats = need;
    }
    lp.roll_newest = (uint32_t) (uintptr_t) a.rows;
    lp.roll_lo = (uint32_t) ((uint64_t) (uintptr_t) a.rows >> 32);
    lp.base_off = (uint32_t) types;
    lp.has_records = (uint32_t) (types >> 32);
    lp.multi = (uint32_t) slots;
    return BF_OK;
}

// BF_FLAG_EXACT_SUM: the handle's limb cells for a launch of `cells` cells, zeroed on `stream` ahead of the launch's first kernel.  The
// buffer is the handle's own and only grows; the renders of one handle are ordered on the device (order_after_last), so one buffer
// serves them all.  The first such launch, or a larger one, allocates: it is then not asynchronous and cannot be captured into a graph.
static bf_status sum_attach(const bf_scene *scene, uint64_t cells, hipStream_t stream) {
    RenderState::Sum &m = scene->run.sum;
    const uint64_t need = std::max<uint64_t>(1, cells);
    if (m.cells < need) {
        if (m.limbs) {
            // as aov_attach grows the side rows: hipFree waits for the device, so an earlier launch that adds to the old cells has ended
            (void) hipFree(m.limbs);
            m.limbs = nullptr;
            m.cells = 0;
        }
        if (hipMalloc(&m.limbs, need * sizeof(int64_t) * bfs::kLimbs) != hipSuccess) {
            (void) hipGetLastError();
            m.limbs = nullptr;
            return fail(BF_ERR_NOMEM, "BF_FLAG_EXACT_SUM: %llu limb cells of %zu bytes cannot be allocated", (unsigned long long) need,
                        sizeof(int64_t) * bfs::kLimbs);
        }
        m.cells = need;
    }
    HIP_TRY(hipMemsetAsync(m.limbs, 0, need * sizeof(int64_t) * bfs::kLimbs, stream));
    return BF_OK;
}

// A render or batch on a handle its caller holds (BF_ENTER).  geom_stride != 0: the batch's renders read per-render geometry
// versions, geom_stride float4 rows apart from the arrays scene->d points at (bf_mesh.cpp: render_versions; kGeom kernels).
bf_status render_locked(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, float *hist_dev,
                        bf_path_record *records_dev, void *stream_, bf_stats *stats_out, uint32_t geom_stride) {
    const uint32_t n_renders = batch ? batch->n_renders : 1u;
    // a device-form vertex update whose gather refused triangles (bf_scene_update_vertices_device) is reported by the handle's
    // next render, once: the render waits for that gather's count (one event, a few bytes) before it enqueues anything
    bf_status st = deform_report(scene, true);
    if (st != BF_OK || (st = check_launch(scene, launch, batch, n_renders, stats_out)) != BF_OK) return st;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    // (more paths than the pool has slots would need several paths per slot and render: not a rolling shape)
    const bool rolling = (launch->flags & BF_FLAG_ROLLING) != 0u && launch->n_paths != 0u &&
                         (uint64_t) n_renders * launch->n_paths <= scene->tun.pool && n_renders <= bfd::kRollRing;
    if ((st = order_after_last(scene, stream)) != BF_OK) return st;
    if (!rolling && (st = close_sequence(scene, stream)) != BF_OK) return st;
    bfd::DLaunch lp;
    if ((st = make_dlaunch(scene, launch, n_renders, geom_stride, stats_out != nullptr, lp)) != BF_OK) return st;
    if (batch && !rolling && (st = stage_batch(scene, launch, batch, stream, lp)) != BF_OK) return st;
    if (rolling) {
        if ((st = wf_roll_render(scene, launch, batch, lp, hist_dev, records_dev, stream)) != BF_OK) return st;
        return mark_last(scene, stream);
    }
    const bool mega = (launch->flags & BF_FLAG_MEGAKERNEL) != 0u;
    // BF_FLAG_EXACT_SUM: the kernels add to the handle's limb cells in place of the caller's floats; the resolve kernel behind the last
    // of them rounds every cell once into hist_dev
    float *const hist_out = hist_dev;
    const bool exact_sum = (launch->flags & BF_FLAG_EXACT_SUM) != 0u;
    if (exact_sum) {
        if ((st = sum_attach(scene, lp.n_chan_all, stream)) != BF_OK) return st;
        hist_dev = reinterpret_cast<float *>(scene->run.sum.limbs);
    }
    // every counter but the sticky guard words (the last ones)
    HIP_TRY(hipMemsetAsync(scene->run.counters, 0, sizeof(unsigned long long) * bfd::CTR_GUARD, stream));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    if (stats_out) {
        HIP_TRY(hipEventCreate(&ev0));
        HIP_TRY(hipEventCreate(&ev1));
        HIP_TRY(hipEventRecord(ev0, stream));
    }
    if (launch->n_paths && mega) {
        // persistent grid: enough workgroups to fill the chip, never more than the work
        const size_t lds = lds_bytes(lp, scene->d.tab_cache, true);
        const uint64_t want = (lp.n_paths + bfd::kBlock - 1) / bfd::kBlock;
        const unsigned blocks_per_cu = (unsigned) std::max<size_t>(1, std::min<size_t>(4, (160 * 1024) / lds));
        const unsigned grid = (unsigned) std::max<uint64_t>(1, std::min<uint64_t>(want, (uint64_t) scene->n_cus * blocks_per_cu));
        // (one side-row slot per thread of the grid)
        if ((launch->flags & BF_FLAG_AOV) && (st = aov_attach(scene, (uint64_t) grid * bfd::kBlock, lp)) != BF_OK) return st;
        HIP_TRY(kernels_for(launch->flags).render(&scene->d, &lp, hist_dev, records_dev, scene->run.counters, (launch->flags & BF_FLAG_STATS) ? 1 : 0,
                                                  grid, lds, stream));
    } else if (launch->n_paths) {
        if ((st = wf_render(scene, kernels_for(launch->flags), lp, hist_dev, records_dev, stream, (launch->flags & BF_FLAG_STATS) != 0,
                            stats_out != nullptr, (launch->flags & BF_FLAG_AOV) != 0u)) != BF_OK) return st;
    }
    if (exact_sum && launch->n_paths) HIP_TRY(bfk_sum_resolve(scene->run.sum.limbs, hist_out, lp.n_chan_all, stream));
    if (stats_out) {
        HIP_TRY(hipEventRecord(ev1, stream));
        HIP_TRY(hipEventSynchronize(ev1));
        if (mega || !launch->n_paths) {      // no wavefront launches: none of their statistics
            RenderState &run = scene->run;
            run.ms[0] = run.ms[1] = run.ms[2] = 0.f;
            run.trace_launches = run.iters = run.tail_launches = run.shade_launches = 0;
        }
        if ((st = read_stats(scene, lp.n_paths, stats_out, launch->n_paths && !mega, ev0, ev1)) != BF_OK) return st;
    }
    return mark_last(scene, stream);
}

static bf_status render_common(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, float *hist_dev,
                               bf_path_record *records_dev, void *stream_, bf_stats *stats_out) {
    if (!scene || !launch || !hist_dev) return fail(BF_ERR_INVALID, "null argument");
    BF_ENTER(scene);
    return render_locked(scene, launch, batch, hist_dev, records_dev, stream_, stats_out);
}

bf_status bf_render_device(const bf_scene *scene, const bf_launch *launch, float *hist_dev, bf_path_record *records_dev,
                           void *stream, bf_stats *stats_out) {
    return render_common(scene, launch, nullptr, hist_dev, records_dev, stream, stats_out);
}

bf_status bf_render_batch_device(const bf_scene *scene, const bf_launch *launch, const bf_batch *batch, float *hist_dev,
                                 bf_path_record *records_dev, void *stream, bf_stats *stats_out) {
    if (!batch) return fail(BF_ERR_INVALID, "bf_render_batch_device: null batch");
    return render_common(scene, launch, batch, hist_dev, records_dev, stream, stats_out);
}

// The handle's AOV table (BF_FLAG_AOV).  It lives on the host alone: every AOV launch carries it in its kernel arguments (aov_attach), so
// "stream-ordered" is the order of the calls that enqueue.
uint32_t bf_aov_floats(uint32_t n_aovs, const uint32_t *types) {
    if (!types || n_aovs == 0 || n_aovs > BF_MAX_AOVS) return 0u;
    uint32_t K = 0;
    for (uint32_t i = 0; i < n_aovs; ++i) {
        if (types[i] >= (uint32_t) BF_AOV_TYPES) return 0u;
        K += bfd::aov_type_floats(types[i]);
    }
    return K;
}

bf_status bf_scene_set_aovs(bf_scene *scene, uint32_t n_aovs, const uint32_t *types, void *stream_) {
    if (!scene) return fail(BF_ERR_INVALID, "bf_scene_set_aovs: null scene");
    if (n_aovs > BF_MAX_AOVS) return fail(BF_ERR_INVALID, "bf_scene_set_aovs: n_aovs %u exceeds BF_MAX_AOVS (%u)", n_aovs, (unsigned) BF_MAX_AOVS);
    if (n_aovs && !types) return fail(BF_ERR_INVALID, "bf_scene_set_aovs: types is null");
    for (uint32_t i = 0; i < n_aovs; ++i)
        if (types[i] >= (uint32_t) BF_AOV_TYPES)
            return fail(BF_ERR_INVALID, "bf_scene_set_aovs: types[%u] = %u is not a BF_AOV_* type (below %u)", i, types[i], (unsigned) BF_AOV_TYPES);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    BF_ENTER(scene);
    // an open rolling sequence ends here, as for bf_scene_set_classes
    bf_status st = order_after_last(scene, stream);
    if (st == BF_OK) st = close_sequence(scene, stream);
    if (st != BF_OK) return st;
    scene->run.aov.n = n_aovs;
    for (uint32_t i = 0; i < n_aovs; ++i) scene->run.aov.types[i] = types[i];
    return BF_OK;
}

bf_status bf_scene_flush(bf_scene *scene, void *stream_, bf_stats *stats_out) {
    if (!scene) return fail(BF_ERR_INVALID, "null argument");
    BF_ENTER(scene);
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    const bool was_open = scene->run.roll.open;
    const uint64_t n_paths = was_open ? scene->run.roll.lp.n_paths : 0;
    bf_status st = order_after_last(scene, stream);
    if (st != BF_OK) return st;
    if (was_open) {
        if ((st = wf_roll_flush(scene, stream, stats_out != nullptr)) != BF_OK) return st;
        if ((st = mark_last(scene, stream)) != BF_OK) return st;
    }
    if (stats_out) {
        std::memset(stats_out, 0, sizeof(*stats_out));
        if (!was_open) return BF_OK;
        HIP_TRY(hipStreamSynchronize(stream));
        return read_stats(scene, n_paths, stats_out, scene->run.roll.lp.count != 0u);       // every path of every render of a COUNTED sequence
    }
    return BF_OK;
}

bf_status bf_scene_sync(bf_scene *scene) {
    if (!scene) return fail(BF_ERR_INVALID, "null argument");
    BF_ENTER(scene);
    bf_status st = close_sequence(scene, scene->run.roll.stream);
    if (st != BF_OK) return st;
    HIP_TRY(scene->run.last.wait());
    scene->run.fb.drop();         // whatever feedback was in flight has landed; the next render re-learns from its own
    // the sticky words of a handle whose work has completed
    unsigned long long g[2] = {0, 0};
    HIP_TRY(hipMemcpy(g, scene->run.counters + bfd::CTR_GUARD, sizeof(g), hipMemcpyDeviceToHost));
    if (g[0] || g[1]) return report_guards(scene, g[0], g[1]);
    return deform_report(scene, true);
}

// ---------------------------------------------------------------------------
// Render until a relative standard error is reached (include/beifong_hip.h: bf_render_converge_device): rounds of
// moment renders accumulated on the device, the statistic of the accumulator after every round (bf_converge.hip), and a stop
// rule that keeps one round in flight ahead of the statistic the host waits for.
// ---------------------------------------------------------------------------
// where the watched pairs of `lm` (BF_FLAG_MOMENT set) sit: the (first, second) pairs of capi.moment_layout, restricted by mode
static bf_status conv_layout(const bf_launch *lm, bfd::ConvLayout &L) {
    std::memset(&L, 0, sizeof(L));
    uint64_t cells = 0;
    if (lm->mode == BF_MODE_RECEIVE_RAW || lm->mode == BF_MODE_RECEIVE_IQ) {
        const bool iq = lm->mode == BF_MODE_RECEIVE_IQ;
        cells = (uint64_t) lm->bins * lm->bins_y;
        L.chan = iq ? 5u : 4u + lm->phase_bins;
        L.pairs = iq ? 2u : 1u;                      // I and Q | Y
        L.first0 = 0u;
        L.second0 = iq ? 3u : 3u + lm->phase_bins;
        L.w_off = 2u;
    } else if (lm->mode <= BF_MODE_TIME) {
        const uint32_t a = lm->mode == BF_MODE_PATH ? 0u : (lm->mode == BF_MODE_RANGE ? lm->bins : 3u * lm->bins);
        cells = multi_pixel_of(lm) ? (uint64_t) lm->film_width * lm->film_height : 1u;
        L.chan = 11u + 2u * a;
        L.pairs = a ? a : 1u;                        // the nested AOVs | nested.Y
        L.first0 = a ? 5u : 6u;
        L.second0 = L.first0 + a + 3u;
        L.w_off = 4u;
    } else {
        return fail(BF_ERR_INVALID, "unknown mode %u", lm->mode);
    }
    L.total = cells * L.chan;
    L.n_pairs = cells * L.pairs;
    if (!L.total || !L.n_pairs) return fail(BF_ERR_INVALID, "the launch has no histogram cells (bins / ADC size 0)");
    // every index the kernels form stays inside a cell, and the cells are the launch's histogram
    if (L.second0 + L.pairs > L.chan || L.total != bf_launch_channels(lm))
        return fail(BF_ERR_DEVICE, "internal: the watched pairs do not fit the moment layout (%u channels per cell)", L.chan);
    return BF_OK;
}

static bool floor_ok(float floor) { return floor >= 0.f && floor <= 1.f; }      // (NaN fails both)

bf_status bf_converge_statistic_device(const bf_launch *launch, const float *hist_dev, float floor, double *stat_out,
                                       uint64_t *n_significant_out, void *stream_) {
    if (!launch || !hist_dev || !stat_out) return fail(BF_ERR_INVALID, "null argument");
    if (!floor_ok(floor)) return fail(BF_ERR_INVALID, "bf_converge_statistic_device: floor %g is outside [0, 1]", (double) floor);
    bf_launch lm = *launch;
    lm.flags |= BF_FLAG_MOMENT;
    bfd::ConvLayout L;
    bf_status st = conv_layout(&lm, L);
    if (st != BF_OK) return st;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    bfd::ConvWork *ws = nullptr;
    bfd::ConvResult *slot = nullptr;
    hipError_t e = hipMalloc((void **) &ws, sizeof(*ws));
    if (e == hipSuccess) e = hipHostMalloc((void **) &slot, sizeof(*slot));
    if (e == hipSuccess) {
        slot->round = ~0u;
        e = bfk_converge_round(const_cast<float *>(hist_dev), nullptr, 0u, &L, (double) floor, ws, slot, 0u, stream);      // (n_blocks 0: read only)
    }
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e == hipSuccess && slot->round != 0u) e = hipErrorUnknown;
    if (e == hipSuccess) {
        *stat_out = slot->stat;
        if (n_significant_out) *n_significant_out = slot->n_significant;
    }
    if (slot) (void) hipHostFree(slot);
    if (ws) (void) hipFree(ws);
    if (e != hipSuccess) return fail(BF_ERR_DEVICE, "bf_converge_statistic_device: %s", hipGetErrorString(e));
    return BF_OK;
}

// the handle's converge state, for rounds of `floats` floats each
static bf_status conv_ensure(const bf_scene *scene, size_t floats) {
    RenderState::Converge &cv = scene->run.conv;
    if (!cv.ws) HIP_TRY(hipMalloc((void **) &cv.ws, sizeof(bfd::ConvWork)));
    if (!cv.ring) HIP_TRY(hipHostMalloc((void **) &cv.ring, RenderState::Converge::kRing * sizeof(bfd::ConvResult)));
    for (hipEvent_t &e : cv.ev)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (cv.cap < floats) {
        // (every earlier converge call has returned behind its last round: nothing reads the old buffers)
        for (float *&q : cv.scratch) {
            if (q) HIP_TRY(hipFree(q));
            q = nullptr;
        }
        cv.cap = 0;
        for (float *&q : cv.scratch) HIP_TRY(hipMalloc((void **) &q, floats * sizeof(float)));
        cv.cap = floats;
    }
    return BF_OK;
}

bf_status bf_render_converge_device(bf_scene *scene, const bf_launch *launch, float target, float floor, uint32_t round_renders,
                                    uint32_t min_rounds, uint32_t max_rounds, float *hist_dev, void *stream_, uint32_t *rounds_out,
                                    double *stat_history_out, uint64_t *n_significant_out, bf_stats *stats_out) {
    const char *fn = "bf_render_converge:";
    if (!scene || !launch || !hist_dev || !rounds_out) return fail(BF_ERR_INVALID, "%s null argument", fn);
    if (launch->flags & BF_FLAG_FAST)
        return fail(BF_ERR_INVALID, "%s BF_FLAG_FAST: the rounds are moment renders, and BF_FLAG_MOMENT | BF_FLAG_FAST is refused", fn);
    if (launch->flags & BF_FLAG_EXACT_SUM)
        return fail(BF_ERR_INVALID, "%s BF_FLAG_EXACT_SUM: the rounds are moment renders, and the exact-sum variants exist of the exact first-moment kernels only", fn);
    if (launch->flags & BF_FLAG_ROLLING) return fail(BF_ERR_INVALID, "%s BF_FLAG_ROLLING: the rounds are batches, which do not roll", fn);
    if (launch->flags & BF_FLAG_CLASSES)
        return fail(BF_ERR_UNSUPPORTED, "%s BF_FLAG_CLASSES: the rounds are moment renders, which have no class variants (per-class error bars are a follow-up)", fn);
    if (launch->flags & BF_FLAG_AOV)
        return fail(BF_ERR_UNSUPPORTED, "%s BF_FLAG_AOV: the rounds are moment renders, which have no AOV variants", fn);
    if (!(target >= 0.f)) return fail(BF_ERR_INVALID, "%s target %g is negative or NaN", fn, (double) target);
    if (!floor_ok(floor)) return fail(BF_ERR_INVALID, "%s floor %g is outside [0, 1]", fn, (double) floor);
    if (round_renders == 0 || max_rounds == 0) return fail(BF_ERR_INVALID, "%s round_renders and max_rounds must be at least 1", fn);
    if (min_rounds > max_rounds) return fail(BF_ERR_INVALID, "%s min_rounds %u exceeds max_rounds %u", fn, min_rounds, max_rounds);
    if (launch->n_paths == 0) return fail(BF_ERR_INVALID, "%s n_paths is 0", fn);
    const bool multi_pixel = multi_pixel_of(launch);
    if (multi_pixel && round_renders > 1)
        return fail(BF_ERR_INVALID, "%s a multi-pixel film is rendered one launch per round (round_renders %u must be 1)", fn, round_renders);
    bf_launch lm = *launch;
    lm.flags |= BF_FLAG_MOMENT;
    BF_ENTER(scene);
    const uint32_t R = round_renders;
    bf_batch batch = {R, nullptr, nullptr};
    // What a render does before it enqueues anything (render_locked), done here before the caller's buffer is touched: a pending
    // report of a device-form vertex update fails the call with hist_dev as it was (it is reported once, so the rounds find none).
    bf_status st = deform_report(scene, true);
    if (st != BF_OK || (st = check_launch(scene, &lm, multi_pixel ? nullptr : &batch, R, nullptr)) != BF_OK) return st;
    bfd::ConvLayout L;
    if ((st = conv_layout(&lm, L)) != BF_OK || (st = conv_ensure(scene, (size_t) R * L.total)) != BF_OK) return st;
    RenderState::Converge &cv = scene->run.conv;
    hipStream_t stream = reinterpret_cast<hipStream_t>(stream_);
    if ((st = order_after_last(scene, stream)) != BF_OK || (st = close_sequence(scene, stream)) != BF_OK) return st;
    if (stats_out) std::memset(stats_out, 0, sizeof(*stats_out));
    HIP_TRY(hipMemsetAsync(hist_dev, 0, L.total * sizeof(float), stream));
    std::vector<uint64_t> seeds(R);
    // round r: its renders into the zeroed scratch, the scratch into the accumulator, the accumulator's statistic into ring slot r
    auto issue = [&](uint32_t r) -> bf_status {
        float *scratch = cv.scratch[r & 1u];
        HIP_TRY(hipMemsetAsync(scratch, 0, (size_t) R * L.total * sizeof(float), stream));
        // Render k = r R + j of the call takes seed launch->seed + k n_paths.  The kernels give path p of a render the stream
        // seed + path_offset + p (bf_path_logic.h: generate_path), so consecutive seeds would render all but one path again; n_paths apart, the
        // renders' streams are the consecutive, disjoint ranges of one render of rounds R n_paths paths (mod 2^64).
        for (uint32_t j = 0; j < R; ++j) seeds[j] = launch->seed + ((uint64_t) r * R + j) * launch->n_paths;
        batch.seeds = seeds.data();
        lm.seed = seeds[0];
        bf_stats rs;
        bf_status s = render_locked(scene, &lm, multi_pixel ? nullptr : &batch, scratch, nullptr, stream_, stats_out ? &rs : nullptr);
        if (s != BF_OK) return s;
        if (stats_out) add_stats(*stats_out, rs);
        HIP_TRY(bfk_converge_round(hist_dev, scratch, R, &L, (double) floor, cv.ws, &cv.ring[r % RenderState::Converge::kRing], r, stream));
        HIP_TRY(hipEventRecord(cv.ev[r & 1u], stream));
        return mark_last(scene, stream);      // (the handle's scratch is in use until here)
    };
    // `limit` rounds are performed: max_rounds until the first statistic at or below the target (round k*, not before round
    // min_rounds - 1) cuts it to k* + 2.  Round r + 1 is in flight whenever stat_r is waited for, so it is part of the result.
    uint32_t limit = max_rounds, issued = 0;
    bool found = false;
    for (; issued < std::min(2u, limit); ++issued)
        if ((st = issue(issued)) != BF_OK) return st;
    for (uint32_t r = 0; r < limit; ++r) {
        HIP_TRY(hipEventSynchronize(cv.ev[r & 1u]));
        const bfd::ConvResult res = cv.ring[r % RenderState::Converge::kRing];
        if (res.round != r) return fail(BF_ERR_DEVICE, "%s the statistic of round %u did not arrive (slot holds round %u)", fn, r, res.round);
        if (stat_history_out) stat_history_out[r] = res.stat;
        if (n_significant_out) *n_significant_out = res.n_significant;
        if (!found && r + 1u >= min_rounds && res.stat <= (double) target) {
            found = true;
            limit = std::min(r + 2u, max_rounds);
        }
        if (issued < limit) {
            if ((st = issue(issued)) != BF_OK) return st;
            ++issued;
        }
    }
    *rounds_out = limit;
    return BF_OK;
}

bf_status bf_render_converge(bf_scene *scene, const bf_launch *launch, float target, float floor, uint32_t round_renders,
                             uint32_t min_rounds, uint32_t max_rounds, float *hist_out, uint32_t *rounds_out,
                             double *stat_history_out, uint64_t *n_significant_out, bf_stats *stats_out) {
    if (!scene || !launch || !hist_out || !rounds_out) return fail(BF_ERR_INVALID, "bf_render_converge: null argument");
    if (launch->flags & BF_FLAG_EXACT_SUM)
        return fail(BF_ERR_INVALID, "bf_render_converge: BF_FLAG_EXACT_SUM: the rounds are moment renders, and the exact-sum variants exist of the exact first-moment kernels only");
    if (launch->flags & BF_FLAG_CLASSES)
        return fail(BF_ERR_UNSUPPORTED, "bf_render_converge: BF_FLAG_CLASSES: the rounds are moment renders, which have no class variants (per-class error bars are a follow-up)");
    if (launch->flags & BF_FLAG_AOV)
        return fail(BF_ERR_UNSUPPORTED, "bf_render_converge: BF_FLAG_AOV: the rounds are moment renders, which have no AOV variants");
    bf_launch lm = *launch;
    lm.flags |= BF_FLAG_MOMENT;
    const size_t bytes = (size_t) bf_launch_channels(&lm) * sizeof(float);
    if (!bytes) return fail(BF_ERR_INVALID, "bf_render_converge: the launch has no histogram cells");
    DeviceGuard on_device(scene->device);
    float *hist_dev = nullptr;
    hipError_t e = hipMalloc((void **) &hist_dev, bytes);
    if (e != hipSuccess) return fail(BF_ERR_NOMEM, "bf_render_converge: hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    bf_status st = bf_render_converge_device(scene, launch, target, floor, round_renders, min_rounds, max_rounds, hist_dev, nullptr, rounds_out,
                                             stat_history_out, n_significant_out, stats_out);
    // (the last round's statistic has been read, so the accumulator is complete; a refused call enqueued nothing)
    if (st == BF_OK) e = hipMemcpy(hist_out, hist_dev, bytes, hipMemcpyDeviceToHost);
    (void) hipFree(hist_dev);
    if (st == BF_OK && e != hipSuccess) return fail(BF_ERR_DEVICE, "bf_render_converge: hipMemcpy: %s", hipGetErrorString(e));
    return st;
}

/* test hook (not part of the ABI): pre-load the sticky guard word, as if wf_trace had dropped `n` rays */
bf_status bfdbg_preload_guard(bf_scene *scene, unsigned long long n) {
    if (!scene) return fail(BF_ERR_INVALID, "null argument");
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(scene->run.counters + bfd::CTR_GUARD, &n, sizeof(n), hipMemcpyHostToDevice));
    return BF_OK;
}

/* test hook (not part of the ABI): waves per SIMD of the build the handle's latest generation launch (the first launch of a pool, the wake
   launch of a rolling call) ran; 0 before any */
bf_status bfdbg_scene_generation_waves(const bf_scene *scene, int *out) {
    if (!scene || !out) return fail(BF_ERR_INVALID, "bfdbg_scene_generation_waves: null argument");
    *out = scene->run.gen_waves_last;
    return BF_OK;
}

}  // extern "C"
