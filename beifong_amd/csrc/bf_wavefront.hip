// Wavefront path tracer for gfx950: the radar hot path as two persistent kernels per bounce iteration over a
// pool of path SLOTS whose state stays in place in HBM (bf_wavefront.h).  There are no queues and no device-wide
// counters on the data path: which slots need work is three 64-bit masks per 64-slot batch (alive / trace /
// shadow), every wave owns a contiguous segment of batches, and a MaskCursor (bf_mask_cursor.h) packs the set bits
// of its segment into full waves on the fly.
//
//   wf_shade : one lane per live slot.  Coalesced state load -> the integrator's vertex logic (emitter hit,
//              Russian roulette, next-event estimation, BSDF sampling: path.cpp:121-209 and the pathlength /
//              pathtime / pathtimefrequency variants, bf_path_logic.h: shade_vertex) -> state stored back in
//              place.  Finished paths are binned (film_put: LDS-privatised histogram) and the slot starts its next
//              path (static assignment: slot i renders paths i, i + n_slots, ...).  New rays are tested here
//              against the analytic rectangles and the four child boxes of the BVH root (presolve_ray); a lane whose
//              rays are all answered that way shades its next vertex in the same visit (up to kShadeChain).
//   wf_trace : persistent waves with dynamic ray replacement walk the four-wide BVH for the rays that do enter
//              the mesh: while-while traversal, 16-entry LDS stack per lane (+ HBM spill), the tree's top 85 nodes
//              in LDS.  Closest hits go to hit[slot]; an occluded shadow ray sets occ[slot].  It reads and writes no
//              other path state: the NEE contribution a shadow ray gates is added by the slot's next reader
//              (kFlagShadowPending, load_state), which loads the state anyway.
//
// The tail of a render (few, long paths) is finished by bf_render_kernel<.., RESUME = true> (bf_kernels.hip).
// All arithmetic is fp32 (the transcendentals are the engine's own fp32 specification, bf_device_math.h; the few
// double operations are where the reference itself multiplies by a double literal, e.g. 1e-9 in phase_update and
// freq_of).  Results are bit-identical per path to the one-kernel variant and to the oracle: same draws, same
// operations in the same order.
#include "bf_film.h"
#include "bf_mask_cursor.h"
#include "bf_launch.h"
#include "bf_variant.h"

#include <utility>

BF_NS_BEGIN

// OR-reduce per-lane bit contributions into the per-batch mask words.  Dense,
// aligned rounds (every lane holds slot batch*64 + lane) store the ballot
// directly; gathered rounds use atomicOr on the (pre-zeroed) words — spread over
// many addresses, non-returning.
BF_DEV void publish_masks(unsigned long long *m_out, bool aligned, bool merge, uint32_t batch0, uint32_t slot, bool valid_lane, bool bit) {
    if (aligned) {
        unsigned long long w = __ballot(bit);
        if ((threadIdx.x & 63) == 0 && w) {
            if (merge)
                atomicOr(&m_out[batch0], w);      // wake launch: wf_shade<0> of the same iteration wrote this word before
            else
                m_out[batch0] = w;
        }
    } else if (valid_lane && bit) {
        atomicOr(&m_out[slot >> 6], 1ull << (slot & 63u));
    }
}

// Early resolution of a freshly spawned ray, done by the shading lane itself
// while the whole wave is active: the analytic rectangles (rectangle.cpp:229-263)
// are tested here, and if the ray misses all child boxes of the BVH root no
// triangle can be hit, so the query is already answered.  Only rays that enter
// the mesh BVH are handed to wf_trace (with the best rectangle hit so far as
// their starting point), which keeps that kernel's waves filled with comparable
// work instead of mixing 3-step misses with 60-step hits.
//   returns true if the ray still needs BVH traversal
BF_DEV bool presolve_ray(const DScene &sc, bool any, V3 o, V3 d, float mint, float maxt, Hit &best, bool &found, const Shift &shf) {
    best.t = BF_INF;
    best.u = best.v = 0.f;
    best.prim = 0;
    best.slot = 0;
    found = false;
    for (uint32_t i = 0; i < sc.n_rects; ++i) {
        CRect &rc = c_rects(sc)[i];
        float t, lx, ly;
        if (rect_intersect(rc, o, d, mint, maxt, t, lx, ly)) {
            if (any) {
                found = true;
                return false;
            }
            consider(best, t, lx, ly, rc.prim, -(int32_t) (i + 1));
        }
    }
    if (sc.n_tris == 0) return false;
    if (sc.root < 0) return true;                 // the whole mesh is one leaf
    // the root node's address is wave-uniform: scalar loads (constant address space, bf_device.h: BF_CAS)
    const c_f4_ptr np = (c_f4_ptr) (uintptr_t) (sc.nodes + 8u * (uint32_t) sc.root);
    const float4 lx = to_float4(np[0]), ly = to_float4(np[1]), lz = to_float4(np[2]), hx = to_float4(np[3]), hy = to_float4(np[4]),
                 hz = to_float4(np[5]), ch = to_float4(np[6]);
    V3 id, oid, ohi;
    ray_inverse_shift(o, d, shf, id, oid, ohi);
    float tmax = any ? maxt : __builtin_fminf(maxt, best.t), tn;
    return slab_fma(lx.x, ly.x, lz.x, hx.x, hy.x, hz.x, id, oid, ohi, mint, tmax, tn) ||
           slab_fma(lx.y, ly.y, lz.y, hx.y, hy.y, hz.y, id, oid, ohi, mint, tmax, tn) ||
           (__float_as_int(ch.z) != kNoNode && slab_fma(lx.z, ly.z, lz.z, hx.z, hy.z, hz.z, id, oid, ohi, mint, tmax, tn)) ||
           (__float_as_int(ch.w) != kNoNode && slab_fma(lx.w, ly.w, lz.w, hx.w, hy.w, hz.w, id, oid, ohi, mint, tmax, tn));
}

// Survivor-area allocation of a wave (rolling sequences, bf_wavefront.h: WF::n_surv).  The wave claims whole survivor
// batches with one returning atomic each and hands their free slots — bits not alive in the parity being consumed; the
// claim is exclusive for the launch — to the lanes that evict a path.  A wave that exhausts its claims (or finds only
// full batches) leaves the remaining paths where they are: they then run late, which is slower, never wrong.
struct SurvAlloc {
    unsigned long long free;    // unclaimed free slots of the current batch (wave-uniform)
    uint32_t batch, claims;
    uint32_t rot;               // claims of the sequence's earlier launches (surv_cursor[0], read once per kernel)
};
BF_DEV void surv_take(const WF &wf, int cur, SurvAlloc &sv, unsigned long long em, bool &evict, uint32_t &dst, int lane) {
    const uint32_t need = (uint32_t) __popcll(em), rank = (uint32_t) __popcll(em & ((1ull << lane) - 1ull));
    const uint32_t main_b = wf.n_main >> 6, surv_b = wf.n_surv >> 6;
    uint32_t served = 0;
    while (served < need) {
        if (sv.free == 0ull) {
            if (sv.claims >= wf.surv_claims_max || surv_b == 0u) break;
            // claim number `nth` of THIS launch (one returning atomic) picks batch (rot + nth) mod surv_b: distinct batches for
            // nth < surv_b whatever the order the waves arrive in.  rot = the claims of all earlier launches of the sequence
            // (surv_cursor[0], constant during the launch: the wake launch that follows folds this launch's count into it), so a
            // launch starts looking where the previous one stopped.
            uint32_t nth = 0;
            if (lane == 0) nth = atomicAdd(wf.surv_cursor + 1, 1u);
            nth = (uint32_t) __shfl((int) nth, 0);
            if (nth >= surv_b) {
                // The launch has handed out every survivor batch once: the next one would be a batch ANOTHER wave of this launch
                // holds, and two waves filling the same free slots lose paths silently (round 3, commit 129745c).  The sizing
                // rule (surv_claims_max x waves <= batches) keeps this from happening; if it ever does, the claim is refused —
                // the paths stay in their slots: slower, never wrong — and counted: the flush / sync of the handle fails.
                if (lane == 0) atomicAdd(&wf.counters[CTR_SURV_GUARD], 1ull);
                sv.claims = wf.surv_claims_max;
                break;
            }
            sv.batch = main_b + (sv.rot + nth) % surv_b;
            sv.free = ~wf.m_alive[cur][sv.batch];
            ++sv.claims;
            continue;
        }
        const uint32_t cnt = (uint32_t) __popcll(sv.free), take = min(need - served, cnt);
        if (evict && rank >= served && rank < served + take) dst = sv.batch * 64u + nth_set_bit(sv.free, rank - served);
        if (take == cnt) {
            sv.free = 0ull;
        } else {
            const uint32_t p = nth_set_bit(sv.free, take - 1u);
            sv.free &= ~((2ull << p) - 1ull);
        }
        served += take;
    }
    if (evict && rank >= served) evict = false;        // no room: the path stays in its slot
}

// wf_shade: one lane per live slot (see the file header of bf_wavefront.h).
//   FIRST = 0 : walk the alive masks of the current parity.
//   FIRST = 1 : bounce 0 of a render (or of a rolling sequence): every slot < n_slots starts its first path.
//   FIRST = 3 : as 0, and paths whose slot is due for its next path move to the survivor area (first launch of a rolling call).
//   FIRST = 2 : "wake" launch of a rolling sequence (bf_render_device with BF_FLAG_ROLLING): the path supply has just
//               grown by one render, so every slot that is NOT alive — it ran out of paths during an earlier call —
//               starts its next path (the one after the last it finished: wf.sd keeps that index for dead slots).
//               The slots that ARE alive belong to wf_shade<0> of the same iteration; both publish into the same
//               next-parity masks.
#ifdef BF_SHADE_PROF
// developer build (tools/shade_profile.py): cycles of the wave between consecutive stamps, by section (the stamps sit in
// wave-uniform control flow); SLP (bf_path_logic.h) counts wave entries and lanes per section
#define SLT(k)                                                            \
    do {                                                                  \
        const unsigned long long slt_now = __builtin_amdgcn_s_memtime();  \
        t_sec[k] += slt_now - slt_last;                                   \
        slt_last = slt_now;                                               \
    } while (0)
#else
#define SLT(k)
#endif
template <int FIRST, int W, int RX>
__global__ __launch_bounds__(kBlock, W) void wf_shade(DScene sc_arg, DLaunch lp, WF wf, uint32_t it, float *__restrict__ g_hist,
                                                      bf_path_record *__restrict__ records) {
    extern __shared__ __align__(16) unsigned char s_raw[];
    float *s_hist = reinterpret_cast<float *>(s_raw);
    const int tid = threadIdx.x, lane = tid & 63;
    DScene sc = sc_arg;
    if (RX & kMulti) sc.tab_cache = 0u;      // several versions of the tables in flight (path_scene): no LDS copy of one of them
    load_tables_lds(sc, (4u * lp.lds_floats + 15u) & ~15u, (uint32_t) tid);      // materials + rectangles behind the histogram
    constexpr bool WALK = FIRST == 0 || FIRST == 3;      // the launch walks the alive masks (else: whole batches of main slots)
    constexpr bool EVICT = FIRST == 3;                   // ... and moves long paths to the survivor area (own variant: the
                                                         // allocator's live values would cost wf_shade<0> its scratch-free build)
    const bool lds_hist = lp.lds_hist != 0;
    if (lp.lds_floats || sc.tab_on) {
        for (uint32_t i = tid; i < lp.lds_floats; i += kBlock) s_hist[i] = 0.f;
        __syncthreads();
    }
    const int cur = it & 1, nxt = cur ^ 1;
    const bool receive = mode_receive<RX>(lp);
    if (FIRST == 2 && blockIdx.x == 0 && tid == 0) {
        // the wake launch follows the evicting launch of its call (same stream): fold that launch's claims into the rotation
        wf.surv_cursor[0] += wf.surv_cursor[1];
        wf.surv_cursor[1] = 0u;
    }
    // the first / wake launches start paths: main slots only (the survivor area never regenerates)
    // (the wake launch: only the batches whose slots are due — the other half of the main slots holds the previous render)
    const uint32_t n_batches = WALK ? wf.n_slots >> 6 : (FIRST == 2 ? wf.wake_nb : wf.n_main >> 6);
    unsigned long long *m_alive = wf.m_alive[nxt], *m_trace = wf.m_trace[nxt], *m_shadow = wf.m_shadow[nxt], *m_hit = wf.m_hit[nxt];
    SurvAlloc sv = {0ull, 0u, 0u, EVICT ? wf.surv_cursor[0] : 0u};

    FilmAcc acc = {0.f, 0.f, 0.f, 0.f, 0.f, 0u, 0u};
    AovCtx av = (RX & kAov) ? aov_ctx(lp) : aov_none();      // kAov: the side rows of the lane's slot (an AOV launch never evicts: the slot is the path's for life)
    uint32_t c_closest = 0, c_shadow = 0, c_bounces = 0, c_live = 0, c_traced = 0, c_loads = 0, c_shq = 0;
#ifdef BF_SHADE_PROF
    const bool lpf = BF_SHADE_PROF >= 2;      // -DBF_SHADE_PROF=2: lane counts per section too (an atomic pair per entry: the cycle shares are then perturbed)
    ShadeProf spf = {0, 0, 0, 0};
    unsigned long long t_sec[8] = {0, 0, 0, 0, 0, 0, 0, 0};     // cursor, load, vertex + film, generate, presolve, chain, store
    unsigned long long slt_last = __builtin_amdgcn_s_memtime();
#endif

    // interleaved share of the batches per wave (MaskCursor; the first / wake launches: batches wave_id, wave_id + n_waves, ...)
    const uint32_t n_waves = gridDim.x * (kBlock / 64), wave_id = blockIdx.x * (kBlock / 64) + (tid >> 6);
    MaskCursor cur_alive;
    // two walks of the alive masks (WF::m_hit): first the slots whose pending vertex is no real hit, then the real hits
    const uint32_t n_pass = (WALK && wf.hit_split) ? 2u : 1u;
    uint32_t first_b = wave_id;
    const bool rolling = lp.roll != nullptr;

    for (uint32_t pass = 0; pass < n_pass; ++pass) {
    if (WALK) cursor_init(cur_alive, wf.m_alive[cur], wave_id, n_waves, n_batches, lane, 1u, n_pass == 2u ? wf.m_hit[cur] : nullptr, pass ? 1u : 2u);
    while (true) {
        // ---- gather up to 64 live slots of the segment into the lanes -----------
        uint32_t slot = 0, got;
        bool aligned;
        if (!WALK) {
            if (first_b >= n_batches) break;
            uint32_t fb = first_b;
            if (FIRST == 2) {
                fb += wf.wake_b0;
                if (fb >= wf.n_main >> 6) fb -= wf.n_main >> 6;
            }
            slot = fb * 64u + lane;
            got = 64;
            aligned = true;
            first_b += n_waves;
        } else {
            cursor_skip_empty(cur_alive, lane);
            if (cursor_empty(cur_alive)) break;
            const uint32_t batch_before = cur_alive.b;
            const bool whole = __popcll(cur_alive.m) == 64;
            got = cursor_take(cur_alive, 64u, true, (uint32_t) lane, slot, lane);
            if (got == 0) break;
            aligned = whole && got == 64 && slot == batch_before * 64u + (uint32_t) lane;
            aligned = __all(aligned);
        }
        bool has = (uint32_t) lane < got;
        if (RX & kAov) av.slot = slot;
        const uint32_t batch0 = slot >> 6;
        // wake: only the slots without a live path — as of NOW: wf_shade<0> of this iteration has run, so a slot whose path
        // ended there, or moved to the survivor area, is free
        if (FIRST == 2) has = ((m_alive[batch0] >> lane) & 1ull) == 0ull;

        PathState s;
        s.render = 0u;                 // lanes without a path still index the batch tables (path_shift)
        ShadowReq sh;
        sh.want = false;
        bool need_gen = false, cont = false, have_hit = false;
        Hit hit;
        hit.t = BF_INF;
        hit.u = hit.v = 0.f;
        hit.prim = 0;
        hit.slot = 0;

        SLP(0, has);
        SLT(0);
        if (has) {
            if (!WALK) {
                need_gen = true;
                // the path BEFORE the one this slot starts now: slot - n_slots for a fresh pool (wraps: + n_slots = slot),
                // the slot's last finished path in a wake launch
                s.path_i = (uint64_t) slot - (uint64_t) wf.n_main;
                if (FIRST == 2) {
                    const uint4 d = wf.sd(slot);
                    s.path_i = ((uint64_t) d.w << 32) | d.z;
                }
            } else {
                float4 hq;
                load_state(wf, slot, receive, s, hq, (RX & kClass) != 0);
                ++c_loads;
                SLP(1, (s.flags & kFlagTermPending) != 0);
                if (s.flags & kFlagTermPending) {
                    // ended after last bounce's BSDF sample; its NEE shadow ray has resolved by now (load_state has added its term)
                    film_put<RX>(sc, lp, s, s_hist, g_hist, lds_hist, acc, records, av);
                    need_gen = true;
                } else {
                    hit.t = hq.x;
                    hit.u = hq.y;
                    hit.v = hq.z;
                    hit.slot = __float_as_int(hq.w);
                    have_hit = true;
                }
            }
        }
#ifdef BF_SHADE_PROF
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
        SLT(1);
        // Chained shading: a lane whose new rays are both answered by the early resolution below
        // (rectangle hit or miss of the mesh, NEE ray clear of the mesh) needs no trace launch, so it
        // shades its next vertex — or starts its next path — right away, up to wf.shade_chain rounds per
        // visit.  Two thirds of all rays resolve that way; each chained round saves a state round trip
        // through HBM and, for paths that leave the scene, a whole bounce iteration.
        bool settled = !has;          // this lane's outcome for the launch is final
        // the slot's path index in wf.sd needs (re)writing if its path ends here: always, except for the idle slots a wake
        // launch finds not due yet (their entry stands); the first launch of a pool writes the initial entries
        bool touched = FIRST != 2;
        bool tracing = false, shadowing = false;
        for (uint32_t round = 0;; ++round) {
            // ---- vertex logic ---------------------------------------------------------------
            SLP(2 + min(round, 2u), !settled && have_hit);
            if (!settled && have_hit) {
                have_hit = false;
#ifdef BF_SHADE_PROF
                cont = shade_vertex<RX>(sc, lp, s, hit, sh, c_bounces, av, &spf, lpf);
#else
                cont = shade_vertex<RX>(sc, lp, s, hit, sh, c_bounces, av);
#endif
                SLT(7);
                SLP(5, !cont);
                if (!cont) {
                    film_put<RX>(sc, lp, s, s_hist, g_hist, lds_hist, acc, records, av);
                    need_gen = true;
                } else if (!(s.flags & kFlagTermPending)) {
                    ++c_closest;
                }
                if (sh.want) ++c_shadow;
            }
            // ---- regeneration: slot i renders paths i, i + n_slots, i + 2 n_slots, ... --------
            // (static assignment: no device-wide path counter to serialise on)
            SLT(2);
            SLP(6, !settled && need_gen);
            if (!settled && need_gen) {
                need_gen = false;
                cont = false;
                const uint64_t path_i = s.path_i + wf.n_main;
                if (slot < wf.n_main && path_i < lp.n_paths) {
                    touched = true;
                    generate_path<RX>(sc, lp, path_i, s);
                    sh.want = false;
                    ++c_closest;
                    cont = true;
                }
            }
            SLT(3);
            // ---- early resolution of the new rays ---------------------------------------------
            if (!settled) {
                tracing = cont && !(s.flags & kFlagTermPending);
                shadowing = cont && sh.want;
                const Shift shf = path_shift(lp, s.render);
                const DScene scp = path_scene<RX>(sc, lp, s.render);      // (kMulti: the rectangles of the path's own render)
                SLP(7, shadowing);
                SLP(8, tracing);
                if (shadowing) {
                    Hit tmp;
                    bool found;
                    if (!presolve_ray(scp, true, sh.o, sh.d, sh.mint, sh.maxt, tmp, found, shf)) {
                        // Scene::sample_emitter_direction zeroes the VALUE of an occluded sample (scene.cpp:220-224) and
                        // the integrator still adds mis * throughput * bsdf * 0: a NaN / inf BSDF value survives that
                        // product.  c * 0 is that term (+-0 for every finite c).
                        s.result += found ? sh.c * 0.f : sh.c;
                        if (receive && lp.iq) s.phase += found ? sh.c_im * 0.f : sh.c_im;
                        shadowing = false;
                    }
                    sh.want = shadowing;
                }
                if (tracing) {
                    bool found;
                    tracing = presolve_ray(scp, false, s.ro, s.rd, s.rmint, s.rmaxt, hit, found, shf);
                }
            }
            SLT(4);
            // ---- chain or settle ----------------------------------------------------------------
            const bool resolved = !settled && cont && !tracing && !shadowing;
            // a resolved REAL hit chains only in company (WF::chain_min): a handful of lanes would run the whole vertex at a
            // fraction of the wave; stored instead, they are shaded packed by the next launch's second pass
            const bool real_hit = !(s.flags & kFlagTermPending) && hit.t != BF_INF;
            const bool lonely = wf.chain_min != 0u && (uint32_t) __popcll(__ballot(resolved && real_hit)) < wf.chain_min;
            const bool chain = resolved && round + 1u < wf.shade_chain && !(lonely && real_hit);
            if (!__any(chain)) break;
            SLP(9, chain && (s.flags & kFlagTermPending));
            SLP(17 + min(round, 2u), chain);
            if (chain) {
                if (s.flags & kFlagTermPending) {
                    // the path ended at its last BSDF sample and its NEE ray is answered: bin it now
                    film_put<RX>(sc, lp, s, s_hist, g_hist, lds_hist, acc, records, av);
                    need_gen = true;
                    cont = false;
                } else {
                    have_hit = true;                    // `hit` is the final answer of the continuation ray
                }
            } else {
                settled = true;
            }
        }
        SLT(5);
        // ---- write back in place ----------------------------------------------------------------
        SLP(20, has && cont);
        SLP(21, has && cont && shadowing);
        // rolling sequence, first launch of a call: a path that goes on while its slot's NEXT path has been supplied moves
        // to the survivor area (its state is in registers anyway: the write-back simply goes to another slot)
        bool evict = false;
        uint32_t dst = slot;
        if (EVICT) {
            // ... and only out of the batches THIS call's wake launch visits (the slots due for the new render's paths): a
            // slot that has fallen behind (the survivor area was full when it was due: its path stayed in place) may sit in the
            // other half of the main slots, and a slot vacated there would stay dead — its pending paths unrendered — until its
            // half is woken again, or for good if the sequence is flushed first (round 4: found by the CTR_FILM check)
            const uint32_t main_b = wf.n_main >> 6, b = slot >> 6;
            const uint32_t rel = b >= wf.wake_b0 ? b - wf.wake_b0 : b + main_b - wf.wake_b0;
            evict = has && cont && slot < wf.n_main && rel < wf.wake_nb && s.path_i + wf.n_main < lp.n_paths;
            const unsigned long long em = __ballot(evict);
            if (em) surv_take(wf, cur, sv, em, evict, dst, lane);
            // the vacated slot's entry names the path that leaves it (the wake launch continues from there): the moved path may
            // have started within this very visit and never been stored here
            if (evict) wf.sd(slot) = make_uint4(0u, 0u, (uint32_t) s.path_i, (uint32_t) (s.path_i >> 32));
        }
        if (has && cont) {
            if (!(s.flags & kFlagTermPending)) {
                // resolved rays carry their final hit; the others start wf_trace from the rectangle hit
                wf.hit(dst) = make_float4(hit.t, hit.u, hit.v, __int_as_float(hit.slot));
                wf.hit_prim(dst) = hit.prim;
            }
            // a shadow ray handed to wf_trace: its term is still missing from s.result (/ s.phase); whoever loads the state next
            // adds it (load_state), with the answer wf_trace leaves in occ
            if (shadowing) s.flags |= kFlagShadowPending;
            store_state(wf, dst, receive, s, (RX & kClass) != 0);
            ++c_live;
            if (shadowing) {
                wf.sh0(dst) = make_float4(sh.o.x, sh.o.y, sh.o.z, sh.mint);
                wf.sh1(dst) = make_float4(sh.d.x, sh.d.y, sh.d.z, sh.maxt);
                wf.sh23(dst) = make_float4(sh.c, (receive && lp.iq) ? sh.c_im : 0.f, __uint_as_float(0u), 0.f);      // sh2, sh3, occ = 0
            }
        } else if (has && rolling && touched) {
            // the slot has run out of paths for now: remember the last one it rendered, so that the wake launch of the
            // sequence's next call continues from there (a path that started and ended within this visit was never stored)
            wf.sd(slot) = make_uint4(0u, 0u, (uint32_t) s.path_i, (uint32_t) (s.path_i >> 32));
        }
        cont = has && cont;
        tracing = cont && tracing;
        shadowing = cont && shadowing;
        publish_masks(m_alive, aligned, FIRST == 2, batch0, slot, has, cont && !evict);
        publish_masks(m_trace, aligned, FIRST == 2, batch0, slot, has, tracing && !evict);
        publish_masks(m_shadow, aligned, FIRST == 2, batch0, slot, has, shadowing && !evict);
        // the hit is final and real (answered by presolve_ray; wf_trace sets the bit for the rays it answers)
        const bool hit_known = cont && !tracing && !(s.flags & kFlagTermPending) && hit.t != BF_INF;
        if (wf.hit_split) publish_masks(m_hit, aligned, FIRST == 2, batch0, slot, has, hit_known && !evict);
        if (evict) {                 // the moved path's bits go to its new slot (the batch's owner ORs its own in as well)
            const unsigned long long bit = 1ull << (dst & 63u);
            atomicOr(&m_alive[dst >> 6], bit);
            if (tracing) atomicOr(&m_trace[dst >> 6], bit);
            if (shadowing) atomicOr(&m_shadow[dst >> 6], bit);
            if (wf.hit_split && hit_known) atomicOr(&m_hit[dst >> 6], bit);
        }
        c_traced += (tracing ? 1u : 0u) + (shadowing ? 1u : 0u);
        c_shq += shadowing ? 1u : 0u;
        SLT(6);
    }
    }

    film_flush<RX>(lp, acc, s_hist, g_hist, lds_hist, tid);
#ifdef BF_SHADE_PROF
    // (the stamps inside shade_vertex sit in divergent code: a lane holds the cycles of the sections IT went through; the
    // wave's figure is the largest)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        spf.si = max(spf.si, (unsigned long long) __shfl_down((long long) spf.si, off));
        spf.head = max(spf.head, (unsigned long long) __shfl_down((long long) spf.head, off));
        spf.nee = max(spf.nee, (unsigned long long) __shfl_down((long long) spf.nee, off));
        spf.bsdf = max(spf.bsdf, (unsigned long long) __shfl_down((long long) spf.bsdf, off));
    }
    if (lane == 0) {
        for (int k = 0; k < 8; ++k) atomicAdd(&g_lane_prof[24 + k], t_sec[k]);      // sections 24..31 of the wave-entry half: cycles
        // inside "vertex + film": surface interaction (incl. the wait for the triangle), head, next-event estimation, BSDF sampling
        atomicAdd(&g_lane_prof[kShadeProfSections + 24], spf.si);
        atomicAdd(&g_lane_prof[kShadeProfSections + 25], spf.head);
        atomicAdd(&g_lane_prof[kShadeProfSections + 26], spf.nee);
        atomicAdd(&g_lane_prof[kShadeProfSections + 27], spf.bsdf);
    }
#endif
    unsigned long long v_closest = c_closest, v_shadow = c_shadow, v_invalid = acc.invalid, v_bounces = c_bounces;
    uint32_t v_live = c_live, v_film = acc.n_put;
    unsigned long long v_traced = c_traced;
    uint32_t v_loads = c_loads, v_shq = c_shq;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        v_loads += __shfl_down(v_loads, off);
        v_shq += __shfl_down(v_shq, off);
        v_traced += __shfl_down(v_traced, off);
        v_closest += __shfl_down(v_closest, off);
        v_shadow += __shfl_down(v_shadow, off);
        v_invalid += __shfl_down(v_invalid, off);
        v_bounces += __shfl_down(v_bounces, off);
        v_live += __shfl_down(v_live, off);
        v_film += __shfl_down(v_film, off);
    }
    // the live count steers the host (never optional): one atomic per WORKGROUP
    __shared__ uint32_t s_live[kBlock / 64];
    if (lane == 0) s_live[tid >> 6] = v_live;
    __syncthreads();
    if (tid == 0) {
        uint32_t t = 0;
        for (int k = 0; k < kBlock / 64; ++k) t += s_live[k];
        if (t) atomicAdd(&wf.n_live[it], t);
    }
    if (lane == 0 && lp.count) {
        if (v_film) atomicAdd(&wf.counters[CTR_FILM], (unsigned long long) v_film);
        if (v_closest) atomicAdd(&wf.counters[CTR_CLOSEST], v_closest);
        if (v_shadow) atomicAdd(&wf.counters[CTR_SHADOW], v_shadow);
        if (v_invalid) atomicAdd(&wf.counters[CTR_INVALID], v_invalid);
        if (v_bounces) atomicAdd(&wf.counters[CTR_BOUNCES], v_bounces);
        if (v_traced) atomicAdd(&wf.counters[CTR_TRACED], v_traced);
        if (v_loads) atomicAdd(&wf.counters[CTR_SHADE_LOADS], (unsigned long long) v_loads);
        if (v_live) atomicAdd(&wf.counters[CTR_SHADE_STORES], (unsigned long long) v_live);
        if (v_shq) atomicAdd(&wf.counters[CTR_SHADE_SHADOW], (unsigned long long) v_shq);
        if (v_closest + v_shadow) atomicAdd(&wf.counters[CTR_SHADE_RAYS], v_closest + v_shadow);
    }
}

// Persistent-wave traversal with dynamic ray replacement.  Each wave owns a
// contiguous segment of batches and walks first their shadow masks (any-hit
// rays) and then their trace masks (closest-hit rays); a lane whose ray has
// finished receives the next set bit as soon as the wave's occupancy drops to
// kRefill lanes (MaskCursor: __popcll / n-th-set-bit select, no atomics), so the
// wave's cost tracks the SUM of its rays' traversal steps instead of 64 x the
// longest one, and sparse pools still traverse with full waves.
//
// "while-while" form: lanes first descend through internal nodes together
// (postponing the leaf they reach), then all lanes holding a leaf intersect
// its triangles together, so the triangle code never runs for one straggler
// while 63 lanes wait at nodes.
//
// Stack: the first kLdsStack entries live in LDS (lane-strided, conflict-free),
// deeper entries — rare: one entry per tree level where BOTH children are hit —
// spill to a per-thread column in HBM.  16 KiB of LDS per workgroup instead of
// 32 lifts the kernel from 5 to 8 waves/SIMD.
constexpr int kLdsStack = 16;
constexpr uint32_t kTraceGuard = 1u << 24;      // wf_trace: inner-loop iterations between two refills (see the guard below)

// GEOM: batched launch with a geometry version per render (WF::geom_stride): a ray walks the nodes and triangles of its own
// render's version.  The LDS copy of the tree's top holds one version, so these rays read the top nodes from memory as well.
template <bool STATS, int W, bool SHIFT, bool QUANT, bool GEOM = false>
__global__ __launch_bounds__(kBlock, W) void wf_trace(DScene sc, WF wf, uint32_t it) {
    __shared__ int s_stack[kLdsStack * kBlock];
    __shared__ float4 s_top[kTopNodes * (QUANT ? kTopStrideQ : kTopStride)];
    int *stack = s_stack + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int nxt = (it & 1) ^ 1;
    uint32_t c_nodes = 0, c_tris = 0, c_top = 0;
    const int n_top = GEOM ? 0 : (int) min(sc.n_nodes, kTopNodes);
    if (QUANT && !GEOM)
        load_top_qnodes(sc.qnodes, (uint32_t) n_top, s_top, threadIdx.x, kBlock);
    else if (!GEOM)
        load_top_nodes(sc.nodes, (uint32_t) n_top, s_top, threadIdx.x, kBlock);
    __syncthreads();
    const uint32_t n_waves = gridDim.x * (kBlock / 64), wave_id = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    LaneStack<kLdsStack, true> st = make_stack<kLdsStack, true>(sc, stack);
    const uint32_t n_batches = wf.n_slots >> 6;
    MaskCursor cursor;
    cursor_init(cursor, wf.m_shadow[nxt], wave_id, n_waves, n_batches, lane);
    bool phase_shadow = true;       // wave-uniform: which job list the cursor walks

    bool has = false, any = false;
    uint32_t job = 0;
    V3 o = mk(0, 0, 0), d = mk(0, 0, 1), id = mk(0, 0, 0), oid = mk(0, 0, 0), ohi = mk(0, 0, 0);
    Shift shf = no_shift();          // SHIFT: batched launch with moving meshes (the ray's render selects the offset)
    uint64_t grows = 0;              // GEOM: float4 rows from render 0's geometry version to the ray's
    float mint = 0.f, maxt = 0.f;
    Hit best;
    best.t = BF_INF;
    best.u = best.v = 0.f;
    best.prim = 0;
    best.slot = 0;
    int node = kNoNode;
    bool found = false;      // any-hit result
    uint32_t guard = 0;

    auto work_left = [&]() -> bool { return phase_shadow || !cursor_empty(cursor); };

    while (true) {
        // ---- refill idle lanes from the wave's segment -------------------------
        unsigned long long idle = __ballot(!has);
        if (idle) {
            uint32_t want = (uint32_t) __popcll(idle);
            const uint32_t rank = (uint32_t) __popcll(idle & ((1ull << lane) - 1ull));
            uint32_t served = 0;
            while (want && work_left()) {
                uint32_t slot = 0;
                const bool req = !has && rank >= served;
                uint32_t got = cursor_take(cursor, want, req, rank - served, slot, lane);
                if (req && rank - served < got) {
                    job = slot;
                    float4 r0, r1;
                    if (phase_shadow) {
                        r0 = wf.sh0(slot);
                        r1 = wf.sh1(slot);
                        any = true;
                    } else {
                        r0 = wf.ray0(slot);
                        r1 = wf.ray1(slot);
                        any = false;
                    }
                    o = mk(r0.x, r0.y, r0.z);
                    d = mk(r1.x, r1.y, r1.z);
                    mint = r0.w;
                    maxt = r1.w;
                    found = false;
                    has = true;
                    best.t = BF_INF;
                    best.u = best.v = 0.f;
                    best.prim = 0;
                    best.slot = 0;
                    if (!phase_shadow) {
                        // closest-hit rays continue from the rectangle hit wf_shade found (presolve_ray)
                        float4 hq = wf.hit(slot);
                        best.t = hq.x;
                        best.u = hq.y;
                        best.v = hq.z;
                        best.slot = __float_as_int(hq.w);
                        best.prim = wf.hit_prim(slot);
                    }
                    if (GEOM) grows = (uint64_t) wf.render(slot) * wf.geom_stride;
                    if (SHIFT) {
                        shf = make_shift(wf.offsets, wf.render(slot), wf.box_slack);
                        ray_inverse_shift(o, d, shf, id, oid, ohi);
                    } else {
                        ray_inverse(o, d, id, oid);
                    }
                    node = sc.root;
                    st.sp = 0;
                }
                served += got;
                want -= got;
                if (want && cursor_empty(cursor) && phase_shadow) {
                    phase_shadow = false;                       // shadow rays done: closest-hit rays next
                    cursor_init(cursor, wf.m_trace[nxt], wave_id, n_waves, n_batches, lane);
                }
            }
        }
        if (__ballot(has) == 0ull) break;
        guard = 0;

        // ---- traversal until the wave thins out -----------------------------------
        while (true) {
            if (++guard > kTraceGuard) {
                // Safety net: a persistent wave must always drain.  The count restarts at every refill, so it bounds the
                // steps ONE set of rays may take (a ray visits each node and leaf at most once: far below the bound).  It
                // is never expected to trip; if it does, the rays are dropped LOUDLY: CTR_GUARD makes bf_render_device
                // fail with BF_ERR_DEVICE (bf_stats.n_guard) instead of returning a plausible histogram.
                const unsigned long long lost = __ballot(has);
                if (lane == 0) atomicAdd(&wf.counters[CTR_GUARD], (unsigned long long) __popcll(lost));
                has = false;
                break;
            }
            // (a) descend through internal nodes; a lane that reaches a leaf (node < 0) waits.
            // Stop descending once fewer than kStragglers lanes are still at internal nodes:
            // they resume after the others' leaves have been intersected.
            while (true) {
                const unsigned long long at_node = __ballot(has && node >= 0);
                if (!at_node) break;
                // progress guarantee: only postpone the stragglers if some lane has a leaf to intersect
                if ((uint32_t) __popcll(at_node) < wf.trace_stragglers && __ballot(has && node < 0 && node != kNoNode)) break;
                if (has && node >= 0) {
                    if (STATS) {
                        ++c_nodes;
                        c_top += node < n_top ? 1u : 0u;
                    }
                    if (QUANT)
                        node = node4q_step_top(GEOM ? sc.qnodes + grows : sc.qnodes, s_top, n_top, node, id, oid, SHIFT ? ohi : oid, mint,
                                               any ? maxt : __builtin_fminf(maxt, best.t), st);
                    else
                        node = node4_step_top(GEOM ? sc.nodes + grows : sc.nodes, s_top, n_top, node, id, oid, SHIFT ? ohi : oid, mint,
                                              any ? maxt : __builtin_fminf(maxt, best.t), st);
                }
            }
            // (b) intersect the postponed leaves together
            if (has && node < 0 && node != kNoNode) {
                if (GEOM) {
                    DScene scg = sc;
                    scg.tris += grows;
                    found = leaf_intersect<STATS>(scg, node, any, o, d, mint, maxt, best, c_tris);
                } else {
                    found = SHIFT ? leaf_intersect<STATS>(sc, node, any, o, d, mint, maxt, best, c_tris, shf)
                                  : leaf_intersect<STATS>(sc, node, any, o, d, mint, maxt, best, c_tris);
                }
                node = found ? kNoNode : st.pop_or_none();
            }
            // (c) retire finished rays
            if (has && node == kNoNode) {
                if (any) {
                    // Scene::ray_test resolved: the one thing the slot's next reader needs to know (load_state adds the term)
                    if (found) wf.occ(job) = 1u;
                } else {
                    wf.hit(job) = make_float4(best.t, best.u, best.v, __int_as_float(best.slot));
                    if (wf.hit_split && best.t != BF_INF) atomicOr(&wf.m_hit[nxt][job >> 6], 1ull << (job & 63u));
                }
                has = false;
            }
            unsigned long long act = __ballot(has);
            if (act == 0ull) break;
            if (work_left() && (uint32_t) __popcll(act) <= wf.trace_refill) break;
        }
    }
    if (STATS) {
        unsigned long long v_nodes = c_nodes, v_tris = c_tris, v_top = c_top;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            v_nodes += __shfl_down(v_nodes, off);
            v_tris += __shfl_down(v_tris, off);
            v_top += __shfl_down(v_top, off);
        }
        if (lane == 0) {
            atomicAdd(&wf.counters[CTR_NODES], v_nodes);
            atomicAdd(&wf.counters[CTR_TRIS], v_tris);
            atomicAdd(&wf.counters[CTR_NODES_LDS], v_top);
        }
    }
}

BF_NS_END  // namespace bfd

#ifdef BF_SHADE_PROF
// developer build: wave entries [0..31] (24..31: cycles between stamps) and lanes [32..63] per section of wf_shade
extern "C" int bfdbg_shade_lane_profile(unsigned long long *out, int clear) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(bfd::g_lane_prof), sizeof(unsigned long long) * 2 * bfd::kShadeProfSections) != hipSuccess) return -1;
    if (clear) {
        void *p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(bfd::g_lane_prof)) != hipSuccess) return -1;
        if (hipMemset(p, 0, sizeof(unsigned long long) * 2 * bfd::kShadeProfSections) != hipSuccess) return -1;
    }
    return 2 * bfd::kShadeProfSections;
}
#endif

static_assert(bfv::kWide == bfd::kWide && bfv::kLean == bfd::kLean && bfv::kMulti == bfd::kMulti && bfv::kGeom == bfd::kGeom &&
                  bfv::kMoment == bfd::kMoment && bfv::kClass == bfd::kClass && bfv::kAov == bfd::kAov && bfv::kSum == bfd::kSum,
              "bf_variant.h restates the variant word of bf_device.h");

namespace {
// f(std::integral_constant<int, C>()) for the one candidate C = AT(0), ..., AT(N - 1) that equals v; false if none does
template <int (*AT)(int), int... Is, class F> bool pick(int v, std::integer_sequence<int, Is...>, F &&f) {
    return ((v == AT(Is) && (f(std::integral_constant<int, AT(Is)>()), true)) || ...);
}
constexpr int itself(int i) { return i; }
}  // namespace

// Which <FIRST, W, V> a shading launch runs is bfv::shade_variant, which of them this object holds is bfv::shade_exists (bf_variant.h):
// the launch's template arguments are the selector's triple, and a triple the object does not hold is refused as a refused launch is.
static hipError_t wf_shade_launch(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it, int first,
                                  float *g_hist, bf_path_record *records, unsigned grid, size_t lds_bytes,
                                  hipStream_t stream, int waves, bfv::Feature feature) {
    const bfv::ShadeForm s = bfv::shade_variant(feature, BF_FAST, bfk_launch_shape(*lp), first, waves);
    bool launched = false;
    pick<itself>(s.first, std::make_integer_sequence<int, bfv::kShadeFirsts>(), [&](auto F) {
        pick<itself>(s.w, std::make_integer_sequence<int, bfv::kShadeWavesMax + 1>(), [&](auto W) {
            pick<bfv::shade_word>(s.v, std::make_integer_sequence<int, bfv::kShadeWords>(), [&](auto V) {
                constexpr int kF = decltype(F)::value, kW = decltype(W)::value, kV = decltype(V)::value;
                if constexpr (bfv::shade_exists(BF_FAST, kF, kW, kV)) {
                    hipLaunchKernelGGL((bfd::wf_shade<kF, kW, kV>), dim3(grid), dim3(bfd::kBlock), lds_bytes, stream, *sc, *lp, *wf, it, g_hist,
                                       records);
                    launched = true;
                }
            });
        });
    });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}
// the families of bf_launch.h this object defines: its own build's (no suffix, or _fast) and, in the exact build, the kMoment
// (BF_FLAG_MOMENT), kClass (BF_FLAG_CLASSES), kAov (BF_FLAG_AOV) and kSum (BF_FLAG_EXACT_SUM) kernels'
#define BF_DEFINE_SHADE_LAUNCHER(name, feature)                                                                                          \
    extern "C" hipError_t bfk_wf_shade##name(const bfd::DScene *sc, const bfd::DLaunch *lp, const bfd::WF *wf, uint32_t it, int first,  \
                                             float *g_hist, bf_path_record *records, unsigned grid, size_t lds_bytes, hipStream_t stream, \
                                             int waves) {                                                                                \
        return wf_shade_launch(sc, lp, wf, it, first, g_hist, records, grid, lds_bytes, stream, waves, feature);                        \
    }
#if BF_FAST
BF_DEFINE_SHADE_LAUNCHER(_fast, bfv::kPlain)
#else
BF_DEFINE_SHADE_LAUNCHER(, bfv::kPlain)
BF_DEFINE_SHADE_LAUNCHER(_moment, bfv::kFeatMoment)
BF_DEFINE_SHADE_LAUNCHER(_class, bfv::kFeatClass)
BF_DEFINE_SHADE_LAUNCHER(_aov, bfv::kFeatAov)
BF_DEFINE_SHADE_LAUNCHER(_sum, bfv::kFeatSum)
#endif
#undef BF_DEFINE_SHADE_LAUNCHER

// bfv::trace_variant and bfv::trace_exists, the same way
extern "C" hipError_t BF_LAUNCHER(bfk_wf_trace)(const bfd::DScene *sc, const bfd::WF *wf, uint32_t it, int stats, unsigned grid,
                                   hipStream_t stream, int waves) {
    const bfv::TraceForm t = bfv::trace_variant(stats != 0, waves, wf->offsets != nullptr, sc->qnodes != nullptr, wf->geom_stride != 0);
    bool launched = false;
    pick<itself>(t.w, std::make_integer_sequence<int, bfv::kTraceWavesMax + 1>(), [&](auto W) {
        pick<itself>(t.flags(), std::make_integer_sequence<int, bfv::kTraceFlags>(), [&](auto B) {
            constexpr bfv::TraceForm k = bfv::trace_form(decltype(W)::value, decltype(B)::value);
            if constexpr (bfv::trace_exists(k)) {
                hipLaunchKernelGGL((bfd::wf_trace<k.stats, k.w, k.shift, k.quant, k.geom>), dim3(grid), dim3(bfd::kBlock), 0, stream, *sc, *wf, it);
                launched = true;
            }
        });
    });
    return launched ? hipGetLastError() : hipErrorInvalidValue;
}
