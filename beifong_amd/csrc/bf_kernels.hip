// Hand-written gfx950 kernels for beifong's transient-radar hot path: the one-kernel estimator loop, the batch
// ray queries, the mesh-translation kernel.
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

#include "bf_path_logic.h"

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

// host-callable launchers (used by bf_api.cpp, bf_render.cpp and bf_mesh.cpp, which are plain C++)
// moment: the kMoment variants (BF_FLAG_MOMENT; the *_moment launchers below); classed: the kClass variants (BF_FLAG_CLASSES; *_class)
static hipError_t render_launch(const bfd::DScene *sc, const bfd::DLaunch *lp, float *g_hist, bf_path_record *records,
                                unsigned long long *counters, int stats, unsigned grid, size_t lds_bytes, hipStream_t stream,
                                bool moment, bool classed = false, bool aov = false) {
    bfd::WF none;
    memset(&none, 0, sizeof(none));
    const bool spill = sc->stack_need > (uint32_t) bfd::kStackDepth;
#if !BF_FAST
    if (moment) {
        // BF_FLAG_MOMENT (never with BF_FLAG_FAST): the kMoment variants of the forms below
#define BF_RENDER_MOM2(S, P, V)                                                                                                        \
    hipLaunchKernelGGL((bfd::bf_render_kernel<S, false, P, BF_TAIL_WAVES, bfd::kMoment | (V)>), dim3(grid), dim3(bfd::kBlock), lds_bytes, \
                       stream, *sc, *lp, g_hist, records, counters, none, 0u)
#define BF_RENDER_MOM(S, P)                                                                    \
    if (lp->geom_stride && lp->wide) BF_RENDER_MOM2(S, P, bfd::kWide | bfd::kGeom);            \
    else if (lp->geom_stride) BF_RENDER_MOM2(S, P, bfd::kGeom);                                \
    else if (lp->wide) BF_RENDER_MOM2(S, P, bfd::kWide);                                       \
    else BF_RENDER_MOM2(S, P, 0)
        if (stats) {
            if (spill) { BF_RENDER_MOM(true, true); }
            else { BF_RENDER_MOM(true, false); }
        } else {
            if (spill) { BF_RENDER_MOM(false, true); }
            else { BF_RENDER_MOM(false, false); }
        }
#undef BF_RENDER_MOM
#undef BF_RENDER_MOM2
        return hipGetLastError();
    }
    if (classed) {
        // BF_FLAG_CLASSES (never with BF_FLAG_FAST or BF_FLAG_MOMENT): the kClass variants of the forms below
#define BF_RENDER_CLS2(S, P, V)                                                                                                       \
    hipLaunchKernelGGL((bfd::bf_render_kernel<S, false, P, BF_TAIL_WAVES, bfd::kClass | (V)>), dim3(grid), dim3(bfd::kBlock), lds_bytes, \
                       stream, *sc, *lp, g_hist, records, counters, none, 0u)
#define BF_RENDER_CLS(S, P)                                                                   \
    if (lp->geom_stride && lp->wide) BF_RENDER_CLS2(S, P, bfd::kWide | bfd::kGeom);           \
    else if (lp->geom_stride) BF_RENDER_CLS2(S, P, bfd::kGeom);                               \
    else if (lp->wide) BF_RENDER_CLS2(S, P, bfd::kWide);                                      \
    else BF_RENDER_CLS2(S, P, 0)
        if (stats) {
            if (spill) { BF_RENDER_CLS(true, true); }
            else { BF_RENDER_CLS(true, false); }
        } else {
            if (spill) { BF_RENDER_CLS(false, true); }
            else { BF_RENDER_CLS(false, false); }
        }
#undef BF_RENDER_CLS
#undef BF_RENDER_CLS2
        return hipGetLastError();
    }
    if (aov) {
        // BF_FLAG_AOV (render modes; never with BF_FLAG_FAST, BF_FLAG_MOMENT or BF_FLAG_CLASSES): the kAov variants of the same forms
        if (lp->mode == BF_MODE_RECEIVE_RAW || lp->roll) return hipErrorInvalidValue;
#define BF_RENDER_AOV2(S, P, V)                                                                                                     \
    hipLaunchKernelGGL((bfd::bf_render_kernel<S, false, P, BF_TAIL_WAVES, bfd::kAov | (V)>), dim3(grid), dim3(bfd::kBlock), lds_bytes, \
                       stream, *sc, *lp, g_hist, records, counters, none, 0u)
#define BF_RENDER_AOV(S, P)                                                                   \
    if (lp->geom_stride && lp->wide) BF_RENDER_AOV2(S, P, bfd::kWide | bfd::kGeom);           \
    else if (lp->geom_stride) BF_RENDER_AOV2(S, P, bfd::kGeom);                               \
    else if (lp->wide) BF_RENDER_AOV2(S, P, bfd::kWide);                                      \
    else BF_RENDER_AOV2(S, P, 0)
        if (stats) {
            if (spill) { BF_RENDER_AOV(true, true); }
            else { BF_RENDER_AOV(true, false); }
        } else {
            if (spill) { BF_RENDER_AOV(false, true); }
            else { BF_RENDER_AOV(false, false); }
        }
#undef BF_RENDER_AOV
#undef BF_RENDER_AOV2
        return hipGetLastError();
    }
#else
    if (moment || classed || aov) return hipErrorInvalidValue;
#endif
#define BF_RENDER_LAUNCH(S, R, P, WF_, IT_)                                                                                              \
    if (lp->wide)                                                                                                                        \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, R, P, BF_TAIL_WAVES, bfd::kWide>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, \
                           *lp, g_hist, records, counters, WF_, IT_);                                                                    \
    else                                                                                                                                 \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, R, P>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, *lp, g_hist,         \
                           records, counters, WF_, IT_)
    if (lp->geom_stride) {
        // per-render geometry versions (bf_render_motion_batch_device)
#define BF_RENDER_GEOM(S, P)                                                                                                          \
    if (lp->wide)                                                                                                                     \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, false, P, BF_TAIL_WAVES, bfd::kWide | bfd::kGeom>), dim3(grid), dim3(bfd::kBlock), \
                           lds_bytes, stream, *sc, *lp, g_hist, records, counters, none, 0u);                                         \
    else                                                                                                                              \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, false, P, BF_TAIL_WAVES, bfd::kGeom>), dim3(grid), dim3(bfd::kBlock), lds_bytes, \
                           stream, *sc, *lp, g_hist, records, counters, none, 0u)
        if (stats) {
            if (spill) { BF_RENDER_GEOM(true, true); }
            else { BF_RENDER_GEOM(true, false); }
        } else {
            if (spill) { BF_RENDER_GEOM(false, true); }
            else { BF_RENDER_GEOM(false, false); }
        }
#undef BF_RENDER_GEOM
        return hipGetLastError();
    }
    if (stats) {
        if (spill) { BF_RENDER_LAUNCH(true, false, true, none, 0u); }
        else { BF_RENDER_LAUNCH(true, false, false, none, 0u); }
    } else {
        if (spill) { BF_RENDER_LAUNCH(false, false, true, none, 0u); }
        else { BF_RENDER_LAUNCH(false, false, false, none, 0u); }
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
static hipError_t tail_launch(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it, uint32_t n_slots,
                              float *g_hist, bf_path_record *records, int stats, size_t lds_bytes, hipStream_t stream,
                              int tail_waves, unsigned spread, unsigned block_cap, bool moment, bool classed = false, bool aov = false) {
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
    const bool spill = sc->stack_need > (uint32_t) bfd::kStackDepth;
    unsigned long long *counters = wf->counters;
    const bool two = tail_waves == 2;
#if !BF_FAST
    if (moment) {
        // BF_FLAG_MOMENT (never with BF_FLAG_FAST): the kMoment variants of the forms below, three waves per SIMD
#define BF_TAIL_MOM2(S, P, V)                                                                                                          \
    hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kMoment | (V)>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, \
                       *lp, g_hist, records, counters, *wf, it)
#define BF_TAIL_MOM(S, P)                                                                      \
    if (lp->geom_stride && lp->wide) BF_TAIL_MOM2(S, P, bfd::kWide | bfd::kGeom);              \
    else if (lp->geom_stride && lp->lean) BF_TAIL_MOM2(S, P, bfd::kLean | bfd::kGeom);         \
    else if (lp->geom_stride) BF_TAIL_MOM2(S, P, bfd::kGeom);                                  \
    else if (lp->multi) BF_TAIL_MOM2(S, P, bfd::kMulti);                                       \
    else if (lp->wide) BF_TAIL_MOM2(S, P, bfd::kWide);                                         \
    else if (lp->lean) BF_TAIL_MOM2(S, P, bfd::kLean);                                         \
    else BF_TAIL_MOM2(S, P, 0)
        if (stats) {
            if (spill) { BF_TAIL_MOM(true, true); }
            else { BF_TAIL_MOM(true, false); }
        } else {
            if (spill) { BF_TAIL_MOM(false, true); }
            else { BF_TAIL_MOM(false, false); }
        }
#undef BF_TAIL_MOM
#undef BF_TAIL_MOM2
        return hipGetLastError();
    }
    if (classed) {
        // BF_FLAG_CLASSES: the kClass variants of the general forms (a lean scene runs the general kernel), three waves per SIMD
        if (lp->multi || lp->roll) return hipErrorInvalidValue;
#define BF_TAIL_CLS2(S, P, V)                                                                                                         \
    hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kClass | (V)>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, \
                       *lp, g_hist, records, counters, *wf, it)
#define BF_TAIL_CLS(S, P)                                                                     \
    if (lp->geom_stride && lp->wide) BF_TAIL_CLS2(S, P, bfd::kWide | bfd::kGeom);             \
    else if (lp->geom_stride) BF_TAIL_CLS2(S, P, bfd::kGeom);                                 \
    else if (lp->wide) BF_TAIL_CLS2(S, P, bfd::kWide);                                        \
    else BF_TAIL_CLS2(S, P, 0)
        if (stats) {
            if (spill) { BF_TAIL_CLS(true, true); }
            else { BF_TAIL_CLS(true, false); }
        } else {
            if (spill) { BF_TAIL_CLS(false, true); }
            else { BF_TAIL_CLS(false, false); }
        }
#undef BF_TAIL_CLS
#undef BF_TAIL_CLS2
        return hipGetLastError();
    }
    if (aov) {
        // BF_FLAG_AOV: the kAov variants of the general forms, three waves per SIMD
        if (lp->mode == BF_MODE_RECEIVE_RAW || lp->roll) return hipErrorInvalidValue;
#define BF_TAIL_AOV2(S, P, V)                                                                                                       \
    hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kAov | (V)>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, \
                       *lp, g_hist, records, counters, *wf, it)
#define BF_TAIL_AOV(S, P)                                                                     \
    if (lp->geom_stride && lp->wide) BF_TAIL_AOV2(S, P, bfd::kWide | bfd::kGeom);             \
    else if (lp->geom_stride) BF_TAIL_AOV2(S, P, bfd::kGeom);                                 \
    else if (lp->wide) BF_TAIL_AOV2(S, P, bfd::kWide);                                        \
    else BF_TAIL_AOV2(S, P, 0)
        if (stats) {
            if (spill) { BF_TAIL_AOV(true, true); }
            else { BF_TAIL_AOV(true, false); }
        } else {
            if (spill) { BF_TAIL_AOV(false, true); }
            else { BF_TAIL_AOV(false, false); }
        }
#undef BF_TAIL_AOV
#undef BF_TAIL_AOV2
        return hipGetLastError();
    }
#else
    if (moment || classed || aov) return hipErrorInvalidValue;
#endif
#define BF_TAIL_LAUNCH(S, P)                                                                                                           \
    if (lp->geom_stride && lp->wide)                                                                                                   \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kWide | bfd::kGeom>), dim3(grid), dim3(bfd::kBlock), lds_bytes,   \
                           stream, *sc, *lp, g_hist, records, counters, *wf, it);                                                      \
    else if (lp->geom_stride && lp->lean)                                                                                              \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kLean | bfd::kGeom>), dim3(grid), dim3(bfd::kBlock), lds_bytes,   \
                           stream, *sc, *lp, g_hist, records, counters, *wf, it);                                                      \
    else if (lp->geom_stride)                                                                                                          \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kGeom>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc,   \
                           *lp, g_hist, records, counters, *wf, it);                                                                   \
    else if (lp->multi)                                                                                                                     \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kMulti>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, \
                           *lp, g_hist, records, counters, *wf, it);                                                                  \
    else if (lp->wide)                                                                                                                      \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kWide>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc,  \
                           *lp, g_hist, records, counters, *wf, it);                                                                  \
    else if (lp->lean && !two)                                                                                                         \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3, bfd::kLean>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc,  \
                           *lp, g_hist, records, counters, *wf, it);                                                                  \
    else if (two)                                                                                                                      \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 2>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, *lp, g_hist, \
                           records, counters, *wf, it);                                                                               \
    else                                                                                                                               \
        hipLaunchKernelGGL((bfd::bf_render_kernel<S, true, P, 3>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, *lp, g_hist, \
                           records, counters, *wf, it)
    if (stats) {
        if (spill) { BF_TAIL_LAUNCH(true, true); }
        else { BF_TAIL_LAUNCH(true, false); }
    } else {
        if (spill) { BF_TAIL_LAUNCH(false, true); }
        else { BF_TAIL_LAUNCH(false, false); }
    }
#undef BF_TAIL_LAUNCH
    return hipGetLastError();
}
extern "C" hipError_t BF_LAUNCHER(bfk_launch_render)(const bfd::DScene *sc, const bfd::DLaunch *lp, float *g_hist, bf_path_record *records,
                                        unsigned long long *counters, int stats, unsigned grid, size_t lds_bytes,
                                        hipStream_t stream) {
    return render_launch(sc, lp, g_hist, records, counters, stats, grid, lds_bytes, stream, false);
}
extern "C" hipError_t BF_LAUNCHER(bfk_launch_tail)(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it,
                                      uint32_t n_slots, float *g_hist, bf_path_record *records, int stats, size_t lds_bytes,
                                      hipStream_t stream, int tail_waves, unsigned spread, unsigned block_cap) {
    return tail_launch(sc, lp, wf, it, n_slots, g_hist, records, stats, lds_bytes, stream, tail_waves, spread, block_cap, false);
}
#if !BF_FAST
extern "C" hipError_t bfk_launch_render_moment(const bfd::DScene *sc, const bfd::DLaunch *lp, float *g_hist, bf_path_record *records,
                                               unsigned long long *counters, int stats, unsigned grid, size_t lds_bytes,
                                               hipStream_t stream) {
    return render_launch(sc, lp, g_hist, records, counters, stats, grid, lds_bytes, stream, true);
}
extern "C" hipError_t bfk_launch_tail_moment(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it,
                                             uint32_t n_slots, float *g_hist, bf_path_record *records, int stats, size_t lds_bytes,
                                             hipStream_t stream, int tail_waves, unsigned spread, unsigned block_cap) {
    return tail_launch(sc, lp, wf, it, n_slots, g_hist, records, stats, lds_bytes, stream, tail_waves, spread, block_cap, true);
}
extern "C" hipError_t bfk_launch_render_class(const bfd::DScene *sc, const bfd::DLaunch *lp, float *g_hist, bf_path_record *records,
                                              unsigned long long *counters, int stats, unsigned grid, size_t lds_bytes,
                                              hipStream_t stream) {
    return render_launch(sc, lp, g_hist, records, counters, stats, grid, lds_bytes, stream, false, true);
}
extern "C" hipError_t bfk_launch_tail_class(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it,
                                            uint32_t n_slots, float *g_hist, bf_path_record *records, int stats, size_t lds_bytes,
                                            hipStream_t stream, int tail_waves, unsigned spread, unsigned block_cap) {
    return tail_launch(sc, lp, wf, it, n_slots, g_hist, records, stats, lds_bytes, stream, tail_waves, spread, block_cap, false, true);
}
extern "C" hipError_t bfk_launch_render_aov(const bfd::DScene *sc, const bfd::DLaunch *lp, float *g_hist, bf_path_record *records,
                                            unsigned long long *counters, int stats, unsigned grid, size_t lds_bytes,
                                            hipStream_t stream) {
    return render_launch(sc, lp, g_hist, records, counters, stats, grid, lds_bytes, stream, false, false, true);
}
extern "C" hipError_t bfk_launch_tail_aov(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it,
                                          uint32_t n_slots, float *g_hist, bf_path_record *records, int stats, size_t lds_bytes,
                                          hipStream_t stream, int tail_waves, unsigned spread, unsigned block_cap) {
    return tail_launch(sc, lp, wf, it, n_slots, g_hist, records, stats, lds_bytes, stream, tail_waves, spread, block_cap, false, false, true);
}
#endif

#if !BF_FAST      // the rest (probes, ray queries, mesh translation, host helpers) exists in the exact build only
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
// bf_scene_pose_morph / bf_render_morph_batch_device: morph targets (blend shapes) of one mesh shape, and the skin
// behind them in the same registers.  One thread per vertex, grid y = version: version v reads its n_targets weights `n_targets`
// floats further (and its bone table `bone_stride` floats further) and writes its vertices `vstride` floats further.
//   p = rest;  for k = 0 .. n_targets-1 in increasing k:  p_c = fl(p_c + fl(w_k d_k,c))    per coordinate, no FMA
//   n likewise from the rest normal and the normal deltas (dnrm == nullptr: the rest normal, bit for bit), not renormalised
//   SKIN: (p, n) then go through skin_blend in place of the skin's own rest arrays
// Every target is always evaluated: a zero weight takes no shortcut.  The deltas lie [target][vertex][3], so a wave's loads for one
// target are contiguous; the weights are indexed by blockIdx.y and the loop counter alone (uniform: scalar loads).  The target loop
// is unrolled four times to keep four targets' loads in flight; the sums are taken in increasing k all the same.  A lane past the
// end computes vertex nv - 1 again and stores nothing, so control flow is uniform up to the barrier.
template <bool SKIN>
__global__ __launch_bounds__(256) void bf_morph_vertices_kernel(const float *__restrict__ rest_pos, const float *__restrict__ rest_nrm,
                                                                const float *__restrict__ dpos, const float *__restrict__ dnrm, uint32_t nv,
                                                                uint32_t n_targets, const float *__restrict__ wts,
                                                                const uint4 *__restrict__ index, const float4 *__restrict__ weight,
                                                                const float *__restrict__ bones, uint32_t n_bones, uint32_t bone_stride,
                                                                float *__restrict__ pos, float *__restrict__ nrm, uint64_t vstride) {
    __shared__ float sb[SKIN ? 256 * 12 : 1];
    const uint32_t v = blockIdx.x * 256u + threadIdx.x, ver = blockIdx.y;
    const bool live = v < nv;
    const size_t vc = 3u * (size_t) (live ? v : nv - 1u), tstride = 3u * (size_t) nv;
    uint4 ix = make_uint4(0u, 0u, 0u, 0u);
    float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
    if (SKIN) {
        ix = index[vc / 3u];
        w = weight[vc / 3u];
        const float *b = bones + (size_t) bone_stride * ver;
        for (uint32_t i = threadIdx.x; i < n_bones * 12u; i += 256u) sb[i] = b[i];
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
    if (SKIN) {
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
// [n_versions][nv][3] each.  bones != nullptr ([n_versions][n_bones][12], device): skinned behind the morph, with `index` and `weight`
extern "C" hipError_t bfk_launch_morph_vertices(const float *rest_pos, const float *rest_nrm, const float *dpos, const float *dnrm, uint32_t nv,
                                                uint32_t n_targets, const float *wts, const uint4 *index, const float4 *weight,
                                                const float *bones, uint32_t n_bones, float *pos, float *nrm, uint32_t n_versions,
                                                hipStream_t stream) {
    if (nv == 0 || n_versions == 0) return hipSuccess;
    if (n_versions > 65535u || n_targets == 0 || n_targets > 256u) return hipErrorInvalidValue;
    const dim3 grid((nv + 255u) / 256u, n_versions);
    if (bones) {
        if (n_bones == 0 || n_bones > 256u || !index || !weight) return hipErrorInvalidValue;
        hipLaunchKernelGGL(bfd::bf_morph_vertices_kernel<true>, grid, dim3(256), 0, stream, rest_pos, rest_nrm, dpos, dnrm, nv, n_targets, wts, index,
                           weight, bones, n_bones, n_bones * 12u, pos, nrm, (uint64_t) 3u * nv);
    } else {
        hipLaunchKernelGGL(bfd::bf_morph_vertices_kernel<false>, grid, dim3(256), 0, stream, rest_pos, rest_nrm, dpos, dnrm, nv, n_targets, wts, index,
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
        // irradiancemeter.cpp:82: the path's sensor weight divides by the surface area (bf_path_logic.h, the same expression)
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
#endif  // !BF_FAST
