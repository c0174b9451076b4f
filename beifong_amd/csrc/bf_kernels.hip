// Hand-written gfx950 kernels for beifong's transient-radar hot path: the one-kernel estimator loop and the wavefront
// pipeline's tail, with their launchers.  The only device file besides bf_wavefront.hip that is built in both arithmetic
// modes (bf_ns.h); the kernels that move geometry are in bf_geom.hip, the batch ray and plugin queries in bf_query.hip.
//
// bf_render_kernel<STATS, RESUME, SPILL> runs the whole estimator loop per lane (generate -> trace -> shade -> ...):
//   RESUME = false : the one-kernel variant of a render (BF_FLAG_MEGAKERNEL, an ablation of the wavefront pipeline
//                    of bf_wavefront.hip): lanes take path indices from wave-local pools of 256 refilled by one
//                    returning atomic, traverse with a 32-entry LDS stack per lane.
//   RESUME = true  : the wavefront pipeline's TAIL.  Once few paths survive, two launches per bounce cost more than
//                    they do; the survivors' slots are adopted through the alive masks and run to completion here.
//                    The tail is latency, not throughput — its length is the longest Russian-roulette survivor's
//                    bounce count times the time of one bounce of a nearly empty wave — so sparse waves trade lanes
//                    for serial depth: one ray per 16-lane DPP row on a sixteen-wide collapse of the same BVH
//                    (traverse_row16: gangs of up to four rows per ray), four lanes per ray on the four-wide tree
//                    (traverse_quad) above that, and idle lanes take over the shadow rays of busy ones.
// Path-length returns are binned into an LDS-privatised histogram flushed with one global atomic per non-empty bin
// per workgroup.  No MFMA: the path is pointer chasing and scalar shading.
//
// Reference semantics (file:line) are cited at each function; the oracle
// (oracle/bf_oracle.cpp) restates the same functions independently on the CPU.
#include <algorithm>
#include <cstring>

#include "bf_film.h"
#include "bf_mask_cursor.h"
#include "bf_launch.h"
#include "bf_variant.h"

BF_NS_BEGIN

// RESUME = false: the whole render in one launch (ablation of the wavefront
// pipeline, BF_FLAG_MEGAKERNEL).
// RESUME = true : the wavefront pipeline's TAIL kernel — once the path supply is
// exhausted and only a few thousand long paths remain, every lane adopts one
// slot of the wavefront queue (state + the closest hit already traced for it)
// and runs that path to completion here, instead of paying two launches per
// bounce for a nearly empty chip.
// Register budget of the tail (waves per SIMD): 3 (168 VGPRs, some scratch) leaves room for the next renders' kernels when
// renders are pipelined over streams; 2 (224 VGPRs, no scratch) is ~10 % faster for the tail itself.  The launcher picks 2
// for small pools (a 2^20-path render never fills the chip: nothing to leave room for) and 3 for large ones.
#ifndef BF_TAIL_WAVES
#define BF_TAIL_WAVES 3
#endif
#ifdef BF_TAIL_PROF
// developer build (make prof): per-wave cycle breakdown of the tail kernel, read back by bfdbg_tail_profile
__device__ unsigned long long g_tail_prof[8192 * 24];
#define BF_PROF_STAMP(var) const unsigned long long var = __builtin_amdgcn_s_memtime()
#else
#define BF_PROF_STAMP(var)
#endif
template <bool STATS, bool RESUME, bool SPILL, int TW = BF_TAIL_WAVES, int VX = 0>
__global__ __launch_bounds__(kBlock, RESUME ? TW : 3) void bf_render_kernel(DScene sc_arg, DLaunch lp, float *__restrict__ g_hist,
                                                           bf_path_record *__restrict__ records,
                                                           unsigned long long *__restrict__ counters, WF wf, uint32_t wf_it) {
    constexpr int kRX = 2 | VX;       // mode class decided at run time; VX: kWide (the filtered put), kLean, kMoment ... (bf_device.h: kernel variant word)
    extern __shared__ __align__(16) unsigned char s_raw[];
    int *s_stack = reinterpret_cast<int *>(s_raw);                         // [kStackDepth][kBlock]
    float *s_hist = reinterpret_cast<float *>(s_raw + sizeof(int) * kStackDepth * kBlock);
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const bool lds_hist = lp.lds_hist != 0;
    DScene sc = sc_arg;
    if (VX & kMulti) sc.tab_cache = 0u;
    load_tables_lds(sc, (uint32_t) (sizeof(int) * kStackDepth * kBlock) + ((4u * lp.lds_floats + 15u) & ~15u), (uint32_t) tid);
    if (lp.lds_floats || sc.tab_on) {
        for (uint32_t i = tid; i < lp.lds_floats; i += kBlock) s_hist[i] = 0.f;
        __syncthreads();
    }
    int *stack = s_stack + tid;
    const bool receive = lp.mode == BF_MODE_RECEIVE_RAW;

    bool alive = false, done = false;
    bool need_closest = false;     // s holds a ray whose hit is not known yet
    bool film = false;             // the path ended at the last shaded vertex; binned after its shadow ray
    ShadowReq sh;
    sh.want = false;
    Hit hit;
    hit.t = BF_INF;
    hit.u = hit.v = 0.f;
    hit.prim = 0;
    hit.slot = 0;
    PathState s;
    s.flags = 0;
    s.render = 0u;                     // lanes without a path still index the batch tables (path_shift)
    s.dlambda = 0.f;
    s.rmint = 0.f;
    s.rmaxt = 0.f;
    FilmAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0u, 0u};
    // kAov: the side rows of the lane's slot — the pool slot it adopts (RESUME), else its own thread of the grid
    AovCtx av = (kRX & kAov) ? aov_ctx(lp) : aov_none();
    if ((kRX & kAov) && !RESUME) av.slot = blockIdx.x * kBlock + (uint32_t) tid;
    uint32_t c_closest = 0, c_shadow = 0, c_nodes = 0, c_wnodes = 0, c_tris = 0, c_bounces = 0;
    // wave-local pool of path indices (uniform across the wave)
    uint64_t pool_next = 0, pool_end = 0;

    // RESUME: this wave's segment of the pool's alive mask; lanes adopt live slots
    // from it whenever they are free (same on-the-fly compaction as wf_shade)
    uint32_t resume_slots = 0;
    bool regen_ok = true;          // RESUME: the adopted slot is a main slot (survivor-area slots of a rolling sequence never regenerate)
    MaskCursor rcur;
    rcur.masks = nullptr;
    rcur.masks2 = nullptr;
    rcur.sel = 0u;
    rcur.b = rcur.b_end = rcur.base = rcur.k = 0;
    rcur.stride = 1u;
    rcur.rot = rcur.inv = rcur.pb = 0u;
    rcur.mod = 0xffffffffu;
    rcur.sub = ~0ull;
    rcur.m = rcur.w = rcur.nz = 0ull;
    if (RESUME) {
        resume_slots = wf.n_main;
        const uint32_t n_batches = wf.n_slots >> 6;
        const uint32_t n_waves = gridDim.x * (kBlock / 64), wave_id = blockIdx.x * (kBlock / 64) + (tid >> 6);
        cursor_init(rcur, wf.m_alive[wf_it & 1], wave_id, n_waves, n_batches, lane, max(1u, wf.tail_share));
    }

#ifdef BF_TAIL_PROF
    unsigned long long pf_iters = 0, pf_regen = 0, pf_trav = 0, pf_film = 0, pf_shade = 0, pf_quad = 0, pf_rowpass = 0;
    unsigned long long pf_dense_iters = 0, pf_dense_trav = 0, pf_dense_shade = 0, pf_dense_rays = 0;
    RowProf pf_row = {0, 0, 0, 0};
    ShadeProf pf_sp = {0, 0, 0, 0};
    const unsigned long long pf_begin = __builtin_amdgcn_s_memtime();
#endif
    while (true) {
        BF_PROF_STAMP(pf_t0);
        // ---- 1. path regeneration: dead lanes pull new path indices -------
        unsigned long long need = __ballot(!alive && !done);
        if (need && RESUME) {
            uint32_t slot = 0;
            const uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
            const uint32_t got = cursor_take(rcur, (uint32_t) __popcll(need), !alive && !done, rank, slot, lane);
            if (!alive && !done) {
                if (rank < got) {
                    float4 hq;
                    load_state(wf, slot, receive, s, hq, (kRX & kClass) != 0);
                    if (kRX & kAov) av.slot = slot;
                    regen_ok = slot < wf.n_main;
                    alive = true;
                    need_closest = false;          // traced (and counted) by wf_trace already
                    film = false;
                    if (!(s.flags & kFlagTermPending)) {
                        hit.t = hq.x;
                        hit.u = hq.y;
                        hit.v = hq.z;
                        hit.slot = __float_as_int(hq.w);
                        hit.prim = 0;
                    }
                } else {
                    done = true;       // the segment has no live slot left for this lane
                }
            }
        } else if (need) {
            uint32_t n_need = __popcll(need);
            uint32_t rank = __popcll(need & ((1ull << lane) - 1ull));
            uint64_t path_i = 0;
            if (pool_end - pool_next < n_need) {
                // refill: one returning atomic per wave for 4 x 64 paths; the old
                // remainder is handed out first, so no index is ever skipped
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(&counters[CTR_NEXT_PATH], 256ull);
                base = __shfl(base, 0);
                uint64_t left = pool_end - pool_next;
                path_i = rank < left ? pool_next + rank : base + (rank - left);
                pool_next = base + (n_need - left);
                pool_end = base + 256ull;
            } else {
                path_i = pool_next + rank;
                pool_next += n_need;
            }
            if (!alive && !done) {
                if (path_i >= lp.n_paths) {
                    done = true;
                } else {
                    generate_path<kRX>(sc, lp, path_i, s);
                    alive = true;
                    need_closest = true;
                    film = false;
                }
            }
        }
        if (__ballot(alive) == 0ull) break;
        BF_PROF_STAMP(pf_t1);

        // ---- 2. traversal phase ------------------------------------------------------
        // Every lane may hold a closest-hit ray (new path, or the continuation ray of the vertex it
        // shaded last iteration) and a shadow ray (NEE of that same vertex).  The two are independent,
        // so lanes that have nothing to trace (their path is over, or the wave's paths have run out —
        // the normal state of the latency-bound tail) take over shadow rays of busy lanes: the wave
        // walks the BVH once per bounce instead of twice.
        const bool term_pending = alive && (s.flags & kFlagTermPending) != 0;
        const bool trace_closest = alive && need_closest && !term_pending;
        const unsigned long long want_mask = __ballot(sh.want);
        bool occluded = false;
        const unsigned long long closest_mask = __ballot(trace_closest);
        const uint32_t n_cl = (uint32_t) __popcll(closest_mask), n_sh = (uint32_t) __popcll(want_mask);
#ifdef BF_TAIL_PROF
        if (RESUME && n_cl + n_sh != 0u && n_cl + n_sh <= 16u) ++pf_quad;
        const bool pf_is_dense = n_cl + n_sh > 16u;
        pf_dense_rays += pf_is_dense ? n_cl + n_sh : 0u;
#endif
        if (RESUME && n_cl + n_sh != 0u && n_cl + n_sh <= wf.row_jobs && sc.wnodes != nullptr) {
            // ---- deep tail: ONE ray per 16-lane row on the sixteen-wide tree (traverse_row16), four rays per pass ------
            // job k < n_cl: closest-hit ray of the k-th lane of closest_mask; job n_cl + k: shadow ray of the k-th lane of
            // want_mask; row r of pass p serves job 4 p + r
            const uint32_t n_jobs = n_cl + n_sh;
            const unsigned long long below = (1ull << lane) - 1ull;
            const uint32_t my_cl_job = (uint32_t) __popcll(closest_mask & below);
            const uint32_t my_sh_job = n_cl + (uint32_t) __popcll(want_mask & below);
            // a lone ray gets all four rows, two rays two rows each (gangs pop several stack entries per step)
            const uint32_t rlog = min(n_jobs == 1u ? 2u : (n_jobs == 2u ? 1u : 0u), sc.wrows_log);
            const uint32_t per_pass = 4u >> rlog, gshift = 4u + rlog;
            for (uint32_t base = 0; base < n_jobs; base += per_pass) {
                const uint32_t job = base + ((uint32_t) lane >> gshift);
                const bool job_active = job < n_jobs;
                const bool job_any = job >= n_cl;
                int src = lane;
                if (job_active) src = (int) (job_any ? nth_set_bit(want_mask, job - n_cl) : nth_set_bit(closest_mask, job));
                const V3 co = mk(__shfl(s.ro.x, src), __shfl(s.ro.y, src), __shfl(s.ro.z, src));
                const V3 cd = mk(__shfl(s.rd.x, src), __shfl(s.rd.y, src), __shfl(s.rd.z, src));
                const float cmint = __shfl(s.rmint, src), cmaxt = __shfl(s.rmaxt, src);
                const V3 so = mk(__shfl(sh.o.x, src), __shfl(sh.o.y, src), __shfl(sh.o.z, src));
                const V3 sd = mk(__shfl(sh.d.x, src), __shfl(sh.d.y, src), __shfl(sh.d.z, src));
                const float smint = __shfl(sh.mint, src), smaxt = __shfl(sh.maxt, src);
                const uint32_t jrender = (uint32_t) __shfl((int) s.render, src);
                const Shift jshift = path_shift(lp, jrender);
                const DScene scj = path_scene<kRX>(sc, lp, jrender);      // (kMulti: the rectangles of the job's render)
                Hit qbest;
                bool qfound;
                traverse_row16<STATS>(scj, rlog, job_active, job_any, job_any ? so : co, job_any ? sd : cd, job_any ? smint : cmint,
                                      job_any ? smaxt : cmaxt, s_stack, qbest, qfound, c_wnodes, c_tris, jshift
#ifdef BF_TAIL_PROF
                                      , pf_row
#endif
                );
#ifdef BF_TAIL_PROF
                ++pf_rowpass;
#endif
                // deliver: closest hits to their lanes, occlusion verdicts to the requesters
                const int cl_lane = (int) (((my_cl_job - base) & (per_pass - 1u)) << gshift);
                const float ht = __shfl(qbest.t, cl_lane), hu = __shfl(qbest.u, cl_lane), hv = __shfl(qbest.v, cl_lane);
                const int hs = __shfl(qbest.slot, cl_lane);
                const uint32_t hp = (uint32_t) __shfl((int) qbest.prim, cl_lane);
                if (trace_closest && my_cl_job >= base && my_cl_job < base + per_pass) {
                    hit.t = ht;
                    hit.u = hu;
                    hit.v = hv;
                    hit.slot = hs;
                    hit.prim = hp;
                    ++c_closest;
                }
                const unsigned long long occl_mask = __ballot(job_active && job_any && qfound);
                if (sh.want && my_sh_job >= base && my_sh_job < base + per_pass) {
                    occluded = (occl_mask >> (((my_sh_job - base) & (per_pass - 1u)) << gshift)) & 1ull;
                    ++c_shadow;
                    // an occluded sample still contributes mis * throughput * bsdf * 0 (scene.cpp:220-224): c * 0
                    s.result += occluded ? sh.c * 0.f : sh.c;
                    if (lp.iq) s.phase += occluded ? sh.c_im * 0.f : sh.c_im;
                    sh.want = false;
                }
            }
        } else if (RESUME && n_cl + n_sh != 0u && n_cl + n_sh <= 16u) {
            // ---- sparse wave (the deep tail): four lanes per ray (traverse_quad) -----------------------
            // job k < n_cl: closest-hit ray of the k-th lane of closest_mask; job n_cl + k: shadow ray of the k-th
            // lane of want_mask; quad k = lanes 4k .. 4k + 3 serves job k
            const uint32_t job = (uint32_t) lane >> 2;
            const bool job_active = job < n_cl + n_sh;
            const bool job_any = job >= n_cl;
            int src = lane;
            if (job_active) src = (int) (job_any ? nth_set_bit(want_mask, job - n_cl) : nth_set_bit(closest_mask, job));
            const V3 co = mk(__shfl(s.ro.x, src), __shfl(s.ro.y, src), __shfl(s.ro.z, src));
            const V3 cd = mk(__shfl(s.rd.x, src), __shfl(s.rd.y, src), __shfl(s.rd.z, src));
            const float cmint = __shfl(s.rmint, src), cmaxt = __shfl(s.rmaxt, src);
            const V3 so = mk(__shfl(sh.o.x, src), __shfl(sh.o.y, src), __shfl(sh.o.z, src));
            const V3 sd = mk(__shfl(sh.d.x, src), __shfl(sh.d.y, src), __shfl(sh.d.z, src));
            const float smint = __shfl(sh.mint, src), smaxt = __shfl(sh.maxt, src);
            const uint32_t jrender = (uint32_t) __shfl((int) s.render, src);
            const Shift jshift = path_shift(lp, jrender);
            const DScene scj = path_scene<kRX>(sc, lp, jrender);
            Hit qbest;
            bool qfound;
            traverse_quad<STATS, SPILL>(scj, job_active, job_any, job_any ? so : co, job_any ? sd : cd, job_any ? smint : cmint,
                                        job_any ? smaxt : cmaxt, s_stack + (tid & ~3), qbest, qfound, c_nodes, c_tris, jshift);
            const unsigned long long below = (1ull << lane) - 1ull;
            // deliver: closest hits to their lanes, occlusion verdicts to the requesters
            const int my_cl_quad = (int) __popcll(closest_mask & below) * 4;
            const float ht = __shfl(qbest.t, my_cl_quad), hu = __shfl(qbest.u, my_cl_quad), hv = __shfl(qbest.v, my_cl_quad);
            const int hs = __shfl(qbest.slot, my_cl_quad);
            const uint32_t hp = (uint32_t) __shfl((int) qbest.prim, my_cl_quad);
            if (trace_closest) {
                hit.t = ht;
                hit.u = hu;
                hit.v = hv;
                hit.slot = hs;
                hit.prim = hp;
                ++c_closest;
            }
            const unsigned long long occl_mask = __ballot(job_active && job_any && qfound);
            if (sh.want) {
                const uint32_t leader = (n_cl + (uint32_t) __popcll(want_mask & below)) * 4u;
                occluded = (occl_mask >> leader) & 1ull;
                ++c_shadow;
                // an occluded sample still contributes mis * throughput * bsdf * 0 (scene.cpp:220-224): c * 0
                s.result += occluded ? sh.c * 0.f : sh.c;
                if (lp.iq) s.phase += occluded ? sh.c_im * 0.f : sh.c_im;
                sh.want = false;
            }
        } else if (want_mask) {
            const unsigned long long free_mask = __ballot(!trace_closest && !sh.want);
            const uint32_t n_del = min((uint32_t) __popcll(want_mask), (uint32_t) __popcll(free_mask));
            const unsigned long long below = (1ull << lane) - 1ull;
            const uint32_t want_rank = (uint32_t) __popcll(want_mask & below), free_rank = (uint32_t) __popcll(free_mask & below);
            const bool delegated = sh.want && want_rank < n_del;
            const bool helper = !trace_closest && !sh.want && free_rank < n_del;
            // helper f serves the f-th requester; requester r is served by the r-th free lane
            const int src = helper ? (int) nth_set_bit(want_mask, free_rank) : lane;
            V3 ho = mk(__shfl(sh.o.x, src), __shfl(sh.o.y, src), __shfl(sh.o.z, src));
            V3 hd = mk(__shfl(sh.d.x, src), __shfl(sh.d.y, src), __shfl(sh.d.z, src));
            const float hmint = __shfl(sh.mint, src), hmaxt = __shfl(sh.maxt, src);
            const uint32_t hrender = (uint32_t) __shfl((int) s.render, src);
            const Shift own_shift = path_shift(lp, s.render), helper_shift = path_shift(lp, hrender);
            const DScene sc_own = path_scene<kRX>(sc, lp, s.render), sc_first = path_scene<kRX>(sc, lp, trace_closest ? s.render : hrender);
            // first walk: closest-hit rays, delegated shadow rays (on their helpers), and the own shadow
            // ray of a lane that has no closest-hit ray to trace
            const bool own_first = sh.want && !delegated && !trace_closest;
            const bool any1 = helper || own_first;
            bool r1 = false;
            if (trace_closest || any1) {
                V3 o1 = trace_closest ? s.ro : ho, d1 = trace_closest ? s.rd : hd;
                float mint1 = trace_closest ? s.rmint : hmint, maxt1 = trace_closest ? s.rmaxt : hmaxt;
                Hit h1;
                r1 = traverse_dyn<STATS, SPILL>(sc_first, any1, o1, d1, mint1, maxt1, stack, h1, c_nodes, c_tris,
                                                trace_closest ? own_shift : helper_shift);
                if (trace_closest) {
                    hit = h1;
                    ++c_closest;
                } else {
                    ++c_shadow;
                }
            }
            const unsigned long long helper_occluded = __ballot(helper && r1);
            if (delegated) occluded = (helper_occluded >> nth_set_bit(free_mask, want_rank)) & 1ull;
            if (own_first) occluded = r1;
            // second walk: lanes that had both rays and found no helper
            const bool own_second = sh.want && !delegated && trace_closest;
            if (__ballot(own_second)) {
                if (own_second) {
                    Hit tmp;
                    occluded = traverse<true, STATS, SPILL>(sc_own, sh.o, sh.d, sh.mint, sh.maxt, stack, tmp, c_nodes, c_tris, own_shift);
                    ++c_shadow;
                }
            }
            if (sh.want) {                                  // occluded: c * 0 (scene.cpp:220-224)
                s.result += occluded ? sh.c * 0.f : sh.c;
                if (lp.iq) s.phase += occluded ? sh.c_im * 0.f : sh.c_im;
            }
            sh.want = false;
        } else if (__ballot(trace_closest)) {
            if (trace_closest) {
                traverse<false, STATS, SPILL>(path_scene<kRX>(sc, lp, s.render), s.ro, s.rd, s.rmint, s.rmaxt, stack, hit, c_nodes, c_tris,
                                              path_shift(lp, s.render));
                ++c_closest;
            }
        }
        if (trace_closest) need_closest = false;
        BF_PROF_STAMP(pf_t2);

        // ---- 3. film: paths that ended at the vertex shaded last iteration (their last shadow ray
        //         has resolved by now) ---------------------------------------------------------------
        if (alive && (film || term_pending)) {
            film_put<kRX>(sc, lp, s, s_hist, g_hist, lds_hist, acc, records, av);
            alive = false;
            film = false;
            if (RESUME) {
                // the slot's static path sequence: i, i + n_slots, i + 2 n_slots, ...
                uint64_t next_path = s.path_i + resume_slots;
                if (regen_ok && next_path < lp.n_paths) {
                    generate_path<kRX>(sc, lp, next_path, s);
                    alive = true;
                    need_closest = true;
                }
            }
        }

        BF_PROF_STAMP(pf_t3);
        // ---- 4. vertex logic for the lanes that hold a fresh hit ---------------------------------
        if (alive && !need_closest) {
            if (!shade_vertex<kRX>(sc, lp, s, hit, sh, c_bounces, av
#ifdef BF_TAIL_PROF
                              , &pf_sp
#endif
                              )) {
                film = true;                                   // ended at the head of the iteration: no new rays
            } else if (s.flags & kFlagTermPending) {
                film = true;                                   // ended by the BSDF sample: its NEE ray is still to trace
            } else {
                need_closest = true;
            }
        }
#ifdef BF_TAIL_PROF
        {
            const unsigned long long pf_t4 = __builtin_amdgcn_s_memtime();
            ++pf_iters;
            if (pf_is_dense) {
                ++pf_dense_iters;
                pf_dense_trav += pf_t2 - pf_t1;
                pf_dense_shade += pf_t4 - pf_t3;
            }
            pf_regen += pf_t1 - pf_t0;
            pf_trav += pf_t2 - pf_t1;
            pf_film += pf_t3 - pf_t2;
            pf_shade += pf_t4 - pf_t3;
        }
#endif
    }
#ifdef BF_TAIL_PROF
    {   // the lane that shaded most vertices (the wave's longest path) speaks for the shading breakdown
        unsigned long long key = pf_sp.si + pf_sp.head + pf_sp.nee + pf_sp.bsdf, best = key;
        for (int off = 32; off > 0; off >>= 1) {
            unsigned long long o = wave_read_u64(best, (lane + off) & 63);
            best = o > best ? o : best;
        }
        best = wave_read_u64(best, 0);
        // after the rotation-reduction lane 0 holds the max over all lanes only if every lane took part: recompute plainly
        unsigned long long m = key;
        for (int off = 1; off < 64; off <<= 1) {
            unsigned long long o = wave_read_u64(m, lane ^ off);
            m = o > m ? o : m;
        }
        const unsigned long long who = __ballot(key == m);
        const int srcl = __ffsll((unsigned long long) who) - 1;
        pf_sp.si = wave_read_u64(pf_sp.si, srcl);
        pf_sp.head = wave_read_u64(pf_sp.head, srcl);
        pf_sp.nee = wave_read_u64(pf_sp.nee, srcl);
        pf_sp.bsdf = wave_read_u64(pf_sp.bsdf, srcl);
        (void) best;
    }
    if (RESUME && lane == 0) {
        const uint32_t w = blockIdx.x * (kBlock / 64) + (tid >> 6);
        if (w < 8192u) {
            unsigned long long *q = g_tail_prof + 24u * w;
            q[16] = pf_dense_iters;
            q[17] = pf_dense_trav;
            q[18] = pf_dense_shade;
            q[19] = pf_dense_rays;
            q[8] = pf_rowpass;
            q[9] = pf_row.steps;
            q[10] = pf_row.rect;
            q[11] = pf_row.mem;
            q[12] = pf_row.cmp;
            q[13] = pf_sp.si;
            q[14] = pf_sp.head;
            q[15] = pf_sp.nee;
            q[7] = pf_sp.bsdf;
            q[0] = pf_iters;
            q[1] = pf_regen;
            q[2] = pf_trav;
            q[3] = pf_film;
            q[4] = pf_shade;
            q[5] = pf_quad;
            q[6] = __builtin_amdgcn_s_memtime() - pf_begin;
        }
    }
#endif

    film_flush<kRX>(lp, acc, s_hist, g_hist, lds_hist, tid);
    // statistics: wave-reduce then one atomic per counter per wave
    unsigned long long v_closest = c_closest, v_shadow = c_shadow, v_nodes = c_nodes, v_tris = c_tris,
                       v_invalid = acc.invalid, v_bounces = c_bounces, v_wnodes = c_wnodes, v_film = acc.n_put;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v_film += __shfl_down(v_film, off);
        v_wnodes += __shfl_down(v_wnodes, off);
        v_closest += __shfl_down(v_closest, off);
        v_shadow += __shfl_down(v_shadow, off);
        v_nodes += __shfl_down(v_nodes, off);
        v_tris += __shfl_down(v_tris, off);
        v_invalid += __shfl_down(v_invalid, off);
        v_bounces += __shfl_down(v_bounces, off);
    }
    if (lane == 0 && lp.count) {
        atomicAdd(&counters[CTR_CLOSEST], v_closest);
        atomicAdd(&counters[CTR_SHADOW], v_shadow);
        if (RESUME) atomicAdd(&counters[CTR_TAIL_RAYS], v_closest + v_shadow);
        if (STATS) {
            atomicAdd(&counters[CTR_NODES], v_nodes + v_wnodes);
            atomicAdd(&counters[CTR_TRIS], v_tris);
            if (RESUME) {
                atomicAdd(&counters[CTR_TAIL_NODES], v_nodes);
                atomicAdd(&counters[CTR_TAIL_WNODES], v_wnodes);
                atomicAdd(&counters[CTR_TAIL_TRIS], v_tris);
            }
        }
        if (RESUME) atomicAdd(&counters[CTR_TAIL_BOUNCES], v_bounces);
        atomicAdd(&counters[CTR_INVALID], v_invalid);
        atomicAdd(&counters[CTR_BOUNCES], v_bounces);
        if (v_film) atomicAdd(&counters[CTR_FILM], v_film);
    }
}

BF_NS_END  // namespace bfd

static_assert(bfv::kWide == bfd::kWide && bfv::kLean == bfd::kLean && bfv::kMulti == bfd::kMulti && bfv::kGeom == bfd::kGeom &&
                  bfv::kMoment == bfd::kMoment && bfv::kClass == bfd::kClass && bfv::kAov == bfd::kAov && bfv::kSum == bfd::kSum,
              "bf_variant.h restates the variant word of bf_device.h");

// host-callable launchers (bf_launch.h; used by bf_render.cpp, which is plain C++)
namespace {
// what every instantiation is launched with (a render passes a zeroed WF and it = 0)
struct KernelLaunch {
    const bfd::DScene *sc;
    const bfd::DLaunch *lp;
    const bfd::WF *wf;
    uint32_t it;
    float *g_hist;
    bf_path_record *records;
    unsigned long long *counters;
    unsigned grid;
    size_t lds_bytes;
    hipStream_t stream;
};
// STATS and SPILL of the form <RESUME, TW, VX>
template <bool RESUME, int TW, int VX> void launch_form(const KernelLaunch &k, int stats) {
#define BF_GO(S, P)                                                                                                                    \
    hipLaunchKernelGGL((bfd::bf_render_kernel<S, RESUME, P, TW, VX>), dim3(k.grid), dim3(bfd::kBlock), k.lds_bytes, k.stream, *k.sc, *k.lp, \
                       k.g_hist, k.records, k.counters, *k.wf, k.it)
    const bool spill = k.sc->stack_need > (uint32_t) bfd::kStackDepth;
    if (stats) {
        if (spill) BF_GO(true, true);
        else BF_GO(true, false);
    } else {
        if (spill) BF_GO(false, true);
        else BF_GO(false, false);
    }
#undef BF_GO
}
}  // namespace

// The one-kernel render.  The cases are the instantiations this object holds: the general kernel with or without per-render geometry
// (bf_render_motion_batch_device) and a wide filter, and in the exact build the same four forms of the kMoment (BF_FLAG_MOMENT),
// kClass (BF_FLAG_CLASSES), kAov (BF_FLAG_AOV) and kSum (BF_FLAG_EXACT_SUM) kernels; none of the four exists in the fast build.
static hipError_t render_launch(const bfd::DScene *sc, const bfd::DLaunch *lp, float *g_hist, bf_path_record *records,
                                unsigned long long *counters, int stats, unsigned grid, size_t lds_bytes, hipStream_t stream,
                                bfv::Feature feature) {
    using namespace bfv;
    bfd::WF none;
    memset(&none, 0, sizeof(none));
    const KernelLaunch k = {sc, lp, &none, 0u, g_hist, records, counters, grid, lds_bytes, stream};
    switch (render_variant(feature, bfk_launch_shape(*lp))) {
        case 0: launch_form<false, BF_TAIL_WAVES, 0>(k, stats); break;
        case kWide: launch_form<false, BF_TAIL_WAVES, kWide>(k, stats); break;
        case kGeom: launch_form<false, BF_TAIL_WAVES, kGeom>(k, stats); break;
        case kWide | kGeom: launch_form<false, BF_TAIL_WAVES, kWide | kGeom>(k, stats); break;
#if !BF_FAST
        case kMoment: launch_form<false, BF_TAIL_WAVES, kMoment>(k, stats); break;
        case kMoment | kWide: launch_form<false, BF_TAIL_WAVES, kMoment | kWide>(k, stats); break;
        case kMoment | kGeom: launch_form<false, BF_TAIL_WAVES, kMoment | kGeom>(k, stats); break;
        case kMoment | kWide | kGeom: launch_form<false, BF_TAIL_WAVES, kMoment | kWide | kGeom>(k, stats); break;
        case kClass: launch_form<false, BF_TAIL_WAVES, kClass>(k, stats); break;
        case kClass | kWide: launch_form<false, BF_TAIL_WAVES, kClass | kWide>(k, stats); break;
        case kClass | kGeom: launch_form<false, BF_TAIL_WAVES, kClass | kGeom>(k, stats); break;
        case kClass | kWide | kGeom: launch_form<false, BF_TAIL_WAVES, kClass | kWide | kGeom>(k, stats); break;
        case kAov: launch_form<false, BF_TAIL_WAVES, kAov>(k, stats); break;
        case kAov | kWide: launch_form<false, BF_TAIL_WAVES, kAov | kWide>(k, stats); break;
        case kAov | kGeom: launch_form<false, BF_TAIL_WAVES, kAov | kGeom>(k, stats); break;
        case kAov | kWide | kGeom: launch_form<false, BF_TAIL_WAVES, kAov | kWide | kGeom>(k, stats); break;
        case kSum: launch_form<false, BF_TAIL_WAVES, kSum>(k, stats); break;
        case kSum | kWide: launch_form<false, BF_TAIL_WAVES, kSum | kWide>(k, stats); break;
        case kSum | kGeom: launch_form<false, BF_TAIL_WAVES, kSum | kGeom>(k, stats); break;
        case kSum | kWide | kGeom: launch_form<false, BF_TAIL_WAVES, kSum | kWide | kGeom>(k, stats); break;
#endif
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// wavefront tail: finish the `n_slots` paths of queue `it` in one launch
//   tail_waves : 3 waves per SIMD (168 VGPRs, some scratch) unless 2 asks for the scratch-free build: alone on the GPU a
//                small pool's tail is 2-3 % faster with 2, but with several renders in flight 3 leave room for the
//                neighbours (C3 0.74 -> 0.69 ms per render, C4 shard 0.96 -> 0.88; profiles/r02_retune_hw_queues.txt)
//   spread     : spread the survivors thinly while the chip has room: a wave that starts with ~16 paths instead of 64
//                runs them four lanes per ray (traverse_quad) from its first bounce and waits for the longest of 16
//   block_cap  : at most this many workgroups (0: no cap)
// The cases: the general, lean, wide and per-path-table (kMulti) kernels, the first three also with per-render geometry, all three
// waves per SIMD, and the general kernel at two; in the exact build the same seven forms of the kMoment kernels and the four
// general forms of the kClass, kAov and kSum kernels (bf_variant.h: tail_variant).
static hipError_t tail_launch(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it, uint32_t n_slots,
                              float *g_hist, bf_path_record *records, int stats, size_t lds_bytes, hipStream_t stream,
                              int tail_waves, unsigned spread, unsigned block_cap, bfv::Feature feature) {
    using namespace bfv;
    // one lane per live slot (gathered from the alive masks), at most one thread per pool slot
    // (any grid finishes the job: waves loop over their segment of the alive masks; the cap keeps the
    // launch within the scene's traversal-spill columns)
    unsigned grid = (std::min(n_slots, wf->n_slots) + bfd::kBlock - 1) / bfd::kBlock;
    {
        const unsigned resident = (sc->spill_stride / bfd::kBlock) * 3u / bfd::kTraceBlocksPerCU;
        if (spread > 1 && grid < resident) grid = std::min(grid * spread, resident);
    }
    grid = std::min(grid, sc->spill_stride / bfd::kBlock);
    if (block_cap) grid = std::min(grid, block_cap);
    if (grid == 0) return hipSuccess;
    const KernelLaunch k = {sc, lp, wf, it, g_hist, records, wf->counters, grid, lds_bytes, stream};
    switch (tail_variant(feature, bfk_launch_shape(*lp, tail_waves))) {
        case 0: launch_form<true, 3, 0>(k, stats); break;
        case kTailTwo: launch_form<true, 2, 0>(k, stats); break;
        case kLean: launch_form<true, 3, kLean>(k, stats); break;
        case kWide: launch_form<true, 3, kWide>(k, stats); break;
        case kMulti: launch_form<true, 3, kMulti>(k, stats); break;
        case kGeom: launch_form<true, 3, kGeom>(k, stats); break;
        case kLean | kGeom: launch_form<true, 3, kLean | kGeom>(k, stats); break;
        case kWide | kGeom: launch_form<true, 3, kWide | kGeom>(k, stats); break;
#if !BF_FAST
        case kMoment: launch_form<true, 3, kMoment>(k, stats); break;
        case kMoment | kLean: launch_form<true, 3, kMoment | kLean>(k, stats); break;
        case kMoment | kWide: launch_form<true, 3, kMoment | kWide>(k, stats); break;
        case kMoment | kMulti: launch_form<true, 3, kMoment | kMulti>(k, stats); break;
        case kMoment | kGeom: launch_form<true, 3, kMoment | kGeom>(k, stats); break;
        case kMoment | kLean | kGeom: launch_form<true, 3, kMoment | kLean | kGeom>(k, stats); break;
        case kMoment | kWide | kGeom: launch_form<true, 3, kMoment | kWide | kGeom>(k, stats); break;
        case kClass: launch_form<true, 3, kClass>(k, stats); break;
        case kClass | kWide: launch_form<true, 3, kClass | kWide>(k, stats); break;
        case kClass | kGeom: launch_form<true, 3, kClass | kGeom>(k, stats); break;
        case kClass | kWide | kGeom: launch_form<true, 3, kClass | kWide | kGeom>(k, stats); break;
        case kAov: launch_form<true, 3, kAov>(k, stats); break;
        case kAov | kWide: launch_form<true, 3, kAov | kWide>(k, stats); break;
        case kAov | kGeom: launch_form<true, 3, kAov | kGeom>(k, stats); break;
        case kAov | kWide | kGeom: launch_form<true, 3, kAov | kWide | kGeom>(k, stats); break;
        case kSum: launch_form<true, 3, kSum>(k, stats); break;
        case kSum | kWide: launch_form<true, 3, kSum | kWide>(k, stats); break;
        case kSum | kGeom: launch_form<true, 3, kSum | kGeom>(k, stats); break;
        case kSum | kWide | kGeom: launch_form<true, 3, kSum | kWide | kGeom>(k, stats); break;
#endif
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// the families of bf_launch.h this object defines: its own build's (no suffix, or _fast) and, in the exact build, the kMoment, kClass,
// kAov and kSum kernels'
#define BF_DEFINE_LAUNCHERS(name, feature)                                                                                              \
    extern "C" hipError_t bfk_launch_render##name(const bfd::DScene *sc, const bfd::DLaunch *lp, float *g_hist, bf_path_record *records, \
                                                  unsigned long long *counters, int stats, unsigned grid, size_t lds_bytes,            \
                                                  hipStream_t stream) {                                                                 \
        return render_launch(sc, lp, g_hist, records, counters, stats, grid, lds_bytes, stream, feature);                              \
    }                                                                                                                                   \
    extern "C" hipError_t bfk_launch_tail##name(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it,          \
                                                uint32_t n_slots, float *g_hist, bf_path_record *records, int stats, size_t lds_bytes,  \
                                                hipStream_t stream, int tail_waves, unsigned spread, unsigned block_cap) {              \
        return tail_launch(sc, lp, wf, it, n_slots, g_hist, records, stats, lds_bytes, stream, tail_waves, spread, block_cap, feature); \
    }
#if BF_FAST
BF_DEFINE_LAUNCHERS(_fast, bfv::kPlain)
#else
BF_DEFINE_LAUNCHERS(, bfv::kPlain)
BF_DEFINE_LAUNCHERS(_moment, bfv::kFeatMoment)
BF_DEFINE_LAUNCHERS(_class, bfv::kFeatClass)
BF_DEFINE_LAUNCHERS(_aov, bfv::kFeatAov)
BF_DEFINE_LAUNCHERS(_sum, bfv::kFeatSum)
#endif
#undef BF_DEFINE_LAUNCHERS

#if !BF_FAST      // the render driver's own small kernel and the developer hooks exist in the exact build only
BF_NS_BEGIN
// one descriptor of a rolling sequence's ring (kernel arguments are captured at launch: no staging buffer to keep alive)
__global__ void bf_roll_set_kernel(DRoll *ring, float4 *offsets, uint32_t idx, DRoll d, float4 off) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        ring[idx] = d;
        offsets[idx] = off;
    }
}
BF_NS_END  // namespace bfd
extern "C" hipError_t bfk_roll_set(bfd::DRoll *ring, float4 *offsets, uint32_t idx, const bfd::DRoll *d, const float *offset3, hipStream_t stream) {
    const float4 off = offset3 ? make_float4(offset3[0], offset3[1], offset3[2], 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
    hipLaunchKernelGGL(bfd::bf_roll_set_kernel, dim3(1), dim3(64), 0, stream, ring, offsets, idx, *d, off);
    return hipGetLastError();
}

#ifdef BF_TAIL_PROF
extern "C" int bfdbg_tail_profile(unsigned long long *out, int n_waves) {
    if (n_waves > 8192) n_waves = 8192;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(bfd::g_tail_prof), sizeof(unsigned long long) * 24 * (size_t) n_waves) != hipSuccess) return -1;
    unsigned long long zero[8] = {0};
    (void) zero;
    return n_waves;
}
extern "C" int bfdbg_tail_profile_clear(void) {
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(bfd::g_tail_prof)) != hipSuccess) return -1;
    return hipMemset(p, 0, sizeof(unsigned long long) * 24 * 8192) == hipSuccess ? 0 : -1;
}
#endif
#endif  // !BF_FAST
