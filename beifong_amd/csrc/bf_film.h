// The film / ADC: what becomes of a finished path's sample, shared verbatim by the wavefront shade kernel (bf_wavefront.hip)
// and the megakernel / tail kernel (bf_kernels.hip):
//
//   film_put   : render_sample / receive_sample tail (integrator.cpp:286, 1590-1665) + the range / time AOVs (range.cpp:141-161,
//                time.cpp:134-153), the phase bins (phase.cpp:93-141), the second moments (moment.cpp:72-91) and the AOV channels
//                (aov.cpp:170-251) + ImageBlock::put / SignalBlock::put: box filter in place (imageblock.cpp:113,166-172,
//                signalblock.cpp:115,162-169), wider filters through put_wide (imageblock.cpp:115-165, signalblock.cpp:117-161)
//                The receive modes' half is film_put_receive, the path's record record_put
//   film_flush : the end of a workgroup's launch: the base channels a wave kept in registers, the LDS-privatised histogram
//                and the workgroup's base-channel tables go to the global histogram (ImageBlock::put(block), imageblock.cpp:56-74)
//                (flush_wave_acc, flush_lds_hist, flush_class_table, flush_sum_table, flush_roll_base, in that order)
#pragma once
#include "bf_device_core.h"
#include "bf_endpoint_logic.h"
#include "bf_path_logic.h"
#include "bf_path_state.h"
#include "bf_sum.h"

BF_NS_BEGIN

// ---------------------------------------------------------------------------
// film / ADC
// ---------------------------------------------------------------------------
// The two destinations are named by address space: through generic pointers the compiler merges both branches into ONE
// flat_atomic_add_f32 on a selected pointer — a vector-memory instruction that finds out per lane whether it addresses LDS
// (round 4: every histogram sample of rounds 1-3 went that way, 20 % of wf_shade's cycles).
typedef __attribute__((address_space(3))) float *lds_float_ptr;
typedef __attribute__((address_space(1))) float *glb_float_ptr;
BF_DEV void lds_add(float *p, float v) {          // ds_add_f32
    (void) __hip_atomic_fetch_add((lds_float_ptr) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
BF_DEV void glb_add(float *p, float v) {          // global_atomic_add_f32
    (void) __hip_atomic_fetch_add((glb_float_ptr) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// kSum (BF_FLAG_EXACT_SUM): a histogram cell is nine int64 limbs (bf_sum.h) and an addend is at most two integer pieces, each added by
// a relaxed vector atomic — ds_add_u64 / global_atomic_add_x2.  Integer addition is associative: whatever order the pieces land in and
// however they are split between LDS and global memory, the limbs hold the exact sum.
typedef __attribute__((address_space(3))) long long *lds_i64_ptr;
typedef __attribute__((address_space(1))) long long *glb_i64_ptr;
BF_DEV void lds_add_i64(long long *p, long long v) {          // ds_add_u64
    (void) __hip_atomic_fetch_add((lds_i64_ptr) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
BF_DEV void glb_add_i64(long long *p, long long v) {          // global_atomic_add_x2
    (void) __hip_atomic_fetch_add((glb_i64_ptr) p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// SUM: s_hist and g_hist address limb arrays, idx counts cells
template <bool SUM = false> BF_DEV void hist_add(float *s_hist, float *g_hist, bool lds, uint32_t idx, float v) {
    if (SUM) {
        const bfs::Pieces p = bfs::split(__float_as_uint(v));
        if (lds) {
            long long *c = reinterpret_cast<long long *>(s_hist) + idx * (uint32_t) bfs::kLimbs + p.limb;
            if (p.lo) lds_add_i64(c, p.lo);
            if (p.hi) lds_add_i64(c + 1, p.hi);
        } else {
            long long *c = reinterpret_cast<long long *>(g_hist) + (size_t) idx * bfs::kLimbs + p.limb;
            if (p.lo) glb_add_i64(c, p.lo);
            if (p.hi) glb_add_i64(c + 1, p.hi);
        }
        return;
    }
    if (lds)
        lds_add(s_hist + idx, v);
    else
        glb_add(g_hist + idx, v);
}
// Where the samples of render `render` go: plain launch = the histogram; batched launch = block `render` of it (LDS and
// global alike); rolling sequence = the render's own histogram (DRoll::hist), privatised in LDS only for the newest
// kRollWindow renders (the few stragglers of older renders take global atomics).  Class launches (kClass; never rolling): block `cls`
// of the render's n_cls blocks, [render][class][n_chan]; n_cls = 0 elsewhere.
struct HistDst {
    float *s, *g;
    bool lds;
};
// kSum launches (SUM; never rolling): the block offset counts cells of bfs::kCellFloats floats each.
template <bool SUM = false>
BF_DEV HistDst hist_dst(const DLaunch &lp, uint32_t render, float *s_hist, float *g_hist, bool lds_hist, uint32_t n_cls = 0u, uint32_t cls = 0u) {
    HistDst h;
    if (lp.roll) {
        h.lds = lds_hist && render >= lp.roll_lo;
        h.g = h.lds ? nullptr : lp.roll[render & (kRollRing - 1u)].hist;      // (no descriptor fetch for the samples that stay in LDS)
        h.s = s_hist + (h.lds ? (render - lp.roll_lo) * lp.n_chan : 0u);
    } else {
        uint32_t hb = lp.batch != 0u ? render * lp.n_chan : 0u;
        if (n_cls) hb = hb * n_cls + cls * lp.n_chan;
        if (SUM) {
            h.g = g_hist + (size_t) hb * bfs::kCellFloats;
            h.s = s_hist + hb * (uint32_t) bfs::kCellFloats;
        } else {
            h.g = g_hist + hb;
            h.s = s_hist + hb;
        }
        h.lds = lds_hist;
    }
    return h;
}

struct FilmAcc {
    float X, Y, Z, A, W;    // base channels of the 1x1 film (render modes)
    uint32_t invalid;
    uint32_t n_put;         // paths binned by this lane (CTR_FILM: the loud "no path was lost" check of the host)
    float nX, nY, nZ;       // kMoment: nested.XYZ (the unweighted result) of the 1x1 film ...
    float qX, qY, qZ;       // ... and their squares (the other variants never touch them: no registers)
};

// ImageBlock::put / SignalBlock::put, the branch for reconstruction filters wider than a pixel (imageblock.cpp:115-165,
// signalblock.cpp:117-161): every channel of the sample goes, times wy * wx, to the cells within `radius` of its position;
// the weights are the host's discretised filter (bf_rfilter), looked up as eval_discretized does (rfilter.h:62-65).
// The sample sits in the block that rendered it: offset `off` (a multiple of bf_rfilter.block_size, integrator.cpp:139-142;
// the ADC is one block), size `bsz`, a border of filt_border cells around it; what lands in the border or outside the
// storage is dropped when the block is added to the film (imageblock.cpp:56-74 put(block): accumulate_2d clips).
struct WideSample {
    float posx, posy;         // pos_ as put() receives it
    int offx, offy;           // block offset
    int bw, bh;               // block size (without border)
    int W, H;                 // storage extent in cells
    int cropx, cropy;         // block coordinate of the storage's first cell (the ADC's window offset; 0 for films)
    uint32_t C;               // channels per cell
    float v0, v1, v2, v3, v4; // base channels (scalars, no indexed array: the hot kernels must stay free of scratch)
    bool five;                // five base channels (render modes) or three (receive modes)
    int ech;                  // channel of the first candidate extra bin (may be negative: that candidate is masked out)
    uint32_t emask;           // candidates that take the sample (bit i: bin i of the three)
    bool e3;                  // three values per bin (time mode) or one
    float e0, e1, e2;
    // kMoment (put_wide<true>): m2_ of a candidate bin sits m2off channels behind it; render modes: nested.XYZ at channel nch,
    // their squares at qch; receive modes: the squares of v0 (and of v1: I/Q) at qch
    uint32_t m2off, nch, qch;
    float n0, n1, n2;
    bool q2;
};
BF_DEV float filt_eval(CSensor &se, float x) {
    const int idx = min((int) __builtin_fabsf(x * se.filt_scale), 31);
    return se.filt_tab[idx];
}
template <bool SUM = false> BF_DEV void put_wide_add(const HistDst &hd, uint32_t idx, float v, float w) {
    const float a = v * w;          // value[k] * weight (imageblock.cpp:160)
    if (a != 0.f) hist_add<SUM>(hd.s, hd.g, hd.lds, idx, a);
}
// (SUM: the kSum variants; never with MOM)
template <bool MOM = false, bool SUM = false> BF_DEV void put_wide(CSensor &se, const WideSample &ws, const HistDst &hd) {
    const int border = (int) se.filt_border, n = (int) se.filt_n;
    const float r = se.filt_radius;
    // pos = pos_ - (m_offset - m_border_size + .5f)
    const float px = ws.posx - ((float) (ws.offx - border) + .5f), py = ws.posy - ((float) (ws.offy - border) + .5f);
    const int sx = ws.bw + 2 * border, sy = ws.bh + 2 * border;
    const int lox = max((int) __builtin_ceilf(px - r), 0), loy = max((int) __builtin_ceilf(py - r), 0);
    const int hix = min((int) __builtin_floorf(px + r), sx - 1), hiy = min((int) __builtin_floorf(py + r), sy - 1);
    const float basex = (float) lox - px, basey = (float) loy - py;
    const int estep = ws.e3 ? 3 : 1;
    for (int yr = 0; yr < n; ++yr) {
        const int y = loy + yr;
        if (y > hiy) break;
        const float wy = filt_eval(se, basey + (float) yr);
        const int gy = ws.offy + y - border - ws.cropy;
        for (int xr = 0; xr < n; ++xr) {
            const int x = lox + xr;
            if (x > hix) break;
            const float w = wy * filt_eval(se, basex + (float) xr);
            const int gx = ws.offx + x - border - ws.cropx;
            if (gx < 0 || gx >= ws.W || gy < 0 || gy >= ws.H) continue;
            const uint32_t cell = ws.C * ((uint32_t) gy * (uint32_t) ws.W + (uint32_t) gx);
            put_wide_add<SUM>(hd, cell + 0u, ws.v0, w);
            put_wide_add<SUM>(hd, cell + 1u, ws.v1, w);
            put_wide_add<SUM>(hd, cell + 2u, ws.v2, w);
            if (ws.five) {
                put_wide_add<SUM>(hd, cell + 3u, ws.v3, w);
                put_wide_add<SUM>(hd, cell + 4u, ws.v4, w);
            }
            for (int i = 0; i < 3; ++i) {
                if (!(ws.emask >> i & 1u)) continue;
                const uint32_t c = cell + (uint32_t) (ws.ech + i * estep);
                put_wide_add<SUM>(hd, c, ws.e0, w);
                if (ws.e3) {
                    put_wide_add<SUM>(hd, c + 1u, ws.e1, w);
                    put_wide_add<SUM>(hd, c + 2u, ws.e2, w);
                }
                if (MOM && ws.five) {          // render modes only: an ADC cell's phase bins have no m2_ channel (Y A W [phase bins] m2_Y)
                    put_wide_add<SUM>(hd, c + ws.m2off, ws.e0 * ws.e0, w);
                    if (ws.e3) {
                        put_wide_add<SUM>(hd, c + ws.m2off + 1u, ws.e1 * ws.e1, w);
                        put_wide_add<SUM>(hd, c + ws.m2off + 2u, ws.e2 * ws.e2, w);
                    }
                }
            }
            if (MOM) {
                if (ws.five) {
                    put_wide_add<SUM>(hd, cell + ws.nch + 0u, ws.n0, w);
                    put_wide_add<SUM>(hd, cell + ws.nch + 1u, ws.n1, w);
                    put_wide_add<SUM>(hd, cell + ws.nch + 2u, ws.n2, w);
                    put_wide_add<SUM>(hd, cell + ws.qch + 0u, ws.n0 * ws.n0, w);
                    put_wide_add<SUM>(hd, cell + ws.qch + 1u, ws.n1 * ws.n1, w);
                    put_wide_add<SUM>(hd, cell + ws.qch + 2u, ws.n2 * ws.n2, w);
                } else {
                    put_wide_add<SUM>(hd, cell + ws.qch, ws.v0 * ws.v0, w);
                    if (ws.q2) put_wide_add<SUM>(hd, cell + ws.qch + 1u, ws.v1 * ws.v1, w);
                }
            }
        }
    }
}
// kAov: the AOV channels of a sample under a wide filter — the same cells and weights as put_wide gives its base channels (the
// footprint arithmetic is put_wide's, statement by statement), value * weight per channel: the table's entries from channel 5 on,
// nested.R G B A at channel `nch`
BF_DEV void put_wide_aov(CSensor &se, const WideSample &ws, const HistDst &hd, const AovCtx &av, const AovVals &a, uint32_t nch, float nested,
                         float alpha) {
    constexpr bool SUM = false;      // (no kAov | kSum kernels)
    const int border = (int) se.filt_border, n = (int) se.filt_n;
    const float r = se.filt_radius;
    const float px = ws.posx - ((float) (ws.offx - border) + .5f), py = ws.posy - ((float) (ws.offy - border) + .5f);
    const int sx = ws.bw + 2 * border, sy = ws.bh + 2 * border;
    const int lox = max((int) __builtin_ceilf(px - r), 0), loy = max((int) __builtin_ceilf(py - r), 0);
    const int hix = min((int) __builtin_floorf(px + r), sx - 1), hiy = min((int) __builtin_floorf(py + r), sy - 1);
    const float basex = (float) lox - px, basey = (float) loy - py;
    for (int yr = 0; yr < n; ++yr) {
        const int y = loy + yr;
        if (y > hiy) break;
        const float wy = filt_eval(se, basey + (float) yr);
        const int gy = ws.offy + y - border - ws.cropy;
        for (int xr = 0; xr < n; ++xr) {
            const int x = lox + xr;
            if (x > hix) break;
            const float w = wy * filt_eval(se, basex + (float) xr);
            const int gx = ws.offx + x - border - ws.cropx;
            if (gx < 0 || gx >= ws.W || gy < 0 || gy >= ws.H) continue;
            const uint32_t cell = ws.C * ((uint32_t) gy * (uint32_t) ws.W + (uint32_t) gx);
            uint32_t ch = cell + 5u;
            for (uint64_t t = av.types; t & 15u; t >>= 4) {
                const uint32_t type = (uint32_t) (t & 15u) - 1u, nf = aov_type_floats(type);
                float vx, vy, vz;
                aov_entry(a, type, vx, vy, vz);
                put_wide_add<SUM>(hd, ch, vx, w);
                if (nf > 1u) put_wide_add<SUM>(hd, ch + 1u, vy, w);
                if (nf > 2u) put_wide_add<SUM>(hd, ch + 2u, vz, w);
                ch += nf;
            }
            put_wide_add<SUM>(hd, cell + nch + 0u, nested, w);
            put_wide_add<SUM>(hd, cell + nch + 1u, nested, w);
            put_wide_add<SUM>(hd, cell + nch + 2u, nested, w);
            put_wide_add<SUM>(hd, cell + nch + 3u, alpha, w);
        }
    }
}
// position_sample of a path's render_sample (integrator.cpp:263): the pixel it was drawn for and the first next_2d of its stream
BF_DEV void film_position(const DLaunch &lp, const PathState &s, uint32_t &px, uint32_t &py, float &fx, float &fy) {
    uint64_t seed = lp.seed, path_offset = lp.path_offset, path_i = s.path_i;
    if (lp.batch != 0u) {
        path_i -= (uint64_t) s.render * lp.batch_paths;
        if (lp.roll) {
            const DRoll &rr = lp.roll[s.render & (kRollRing - 1u)];
            seed = rr.seed;
            path_offset = rr.path_offset;
        } else if (lp.batch_seeds) {
            seed = lp.batch_seeds[s.render];
        }
    }
    Rng rng;
    pcg_seed(rng, seed + path_offset + path_i);
    fx = next_1d(rng);
    fy = next_1d(rng);
    px = py = 0u;
    if (lp.spp) {
        const uint64_t q = (lp.path_offset + path_i) / lp.spp;
        px = (uint32_t) (q % lp.film_w);
        py = (uint32_t) (q / lp.film_w);
    }
}

// SignalBlock::put of a receive mode's sample; hands back what the path's record takes
template <int RX>
BF_DEV void film_put_receive(const DScene &sc, const DLaunch &lp, const PathState &s, const HistDst &hd, bool valid, FilmAcc &acc,
                             float &rec_L, float &rec_aux) {
    float *const s_hist = hd.s, *const g_hist = hd.g;
    const bool lds_hist = hd.lds;
    constexpr bool wide = (RX & kWide) != 0;       // reconstruction filter wider than a pixel (uniform; the radar scenes use box)
    constexpr bool mom = (RX & kMoment) != 0;      // BF_FLAG_MOMENT: second moments next to every first-moment channel (beifong_hip.h)
    constexpr bool sum = (RX & kSum) != 0;         // BF_FLAG_EXACT_SUM: the cells are limbs (hist_add)
    // receive_sample tail — integrator.cpp:1625-1665; SignalBlock::put — signalblock.cpp:162-169
    CSensor &se = c_sensor(sc);
    float tf0 = s.t_rx - se.adc_sampling_start;
    float tf1 = freq_of(sc.c, rare<RX>(lp.doppler != 0u) ? s.lambda0 + s.dlambda : s.lambda0);
    // "mix_resample": |f_after - f_rx| (integrator.cpp:1590-1601); with a re-sampling transmitter lambda0 is the wavelength the
    // path ENDS with (ray_.wavelengths = si.wavelengths, pathtimefrequency.cpp:451) and dlambda the one the receiver drew
    if (rare<RX>(lp.mix != 0u)) tf1 = __builtin_fabsf(tf1 - freq_of(sc.c, rare<RX>(lp.resample != 0u) ? s.dlambda : s.lambda0));
    tf0 *= (float) se.t_bins / se.t_bandwidth;
    tf1 *= (float) se.f_bins / se.f_bandwidth;
    float L = __builtin_fabsf(s.aux) * s.result;          // aux holds ray_weight in receive mode
    float a0 = valid ? 4.f * L : 0.f;                     // hsum over 4 identical spectral lanes
    float a1 = valid ? 1.f : 0.f;
    if (lp.iq) a1 = valid ? 4.f * (__builtin_fabsf(s.aux) * s.phase) : 0.f;   // I, Q, W instead of Y, A, W
    bool ok = __builtin_isfinite(a0) && __builtin_isfinite(a1);
    // moment cells: Y A W [phase bins] m2_Y, or I Q W m2_I m2_Q; a square that is not finite drops the sample
    const float q0 = mom ? a0 * a0 : 0.f, q1 = (mom && lp.iq) ? a1 * a1 : 0.f;
    if (mom) ok = ok && __builtin_isfinite(q0) && __builtin_isfinite(q1);
    // PhaseIntegrator::sample (phase.cpp:93-141): S{k}.Y takes hsum(L), before the receiver weight,
    // iff rect((phase - centre_k) / width) > 0; evaluated exactly as written there for the (at most
    // three) candidate bins around phase / width
    const uint32_t P = (RX & kLean) ? 0u : lp.phase_bins;
    const float pv = valid ? 4.f * s.result : 0.f;
    int pk0 = 0;
    uint32_t pmask = 0u;            // bit i: bin pk0 - 1 + i takes the sample
    if (P) {
        const float two_pi = 6.28318530717958647692f;
        const float width = two_pi / (float) (int) P;
        float phase = __builtin_fmodf(valid ? 0.f + s.phase : 0.f, two_pi);
        phase += (phase < 0.f) ? two_pi : 0.f;
        const float fk = __builtin_floorf(phase / width);             // NaN phases (a miss: -inf) select no bin
        pk0 = (fk >= 0.f && fk < (float) P) ? (int) fk : ((fk >= (float) P) ? (int) P - 1 : 0);
        for (int i = 0; i < 3; ++i) {
            const int k = pk0 - 1 + i;
            if (k < 0 || k >= (int) P) continue;
            float centre = (float) ((double) width * ((double) k + 0.5));
            if (jabs((phase - centre) / width) < 0.5f) pmask |= 1u << i;
        }
        ok = ok && __builtin_isfinite(pv);
    }
    // pos = tf - (m_offset - m_border_size + .5f), lo = ceil(pos - .5f) (signalblock.cpp:115,163): the block sits at the ADC's
    // window offset (integrator.cpp:627; 0 without a window), the histogram is the window
    const uint32_t wot = rare<RX>(se.win_off_t != 0u) ? se.win_off_t : 0u, wof = rare<RX>(se.win_off_f != 0u) ? se.win_off_f : 0u;
    float lx = __builtin_ceilf((tf0 - ((float) wot + .5f)) - .5f), ly = __builtin_ceilf((tf1 - ((float) wof + .5f)) - .5f);
    if (wide) {
        if (ok) {
            WideSample ws;
            ws.posx = tf0;
            ws.posy = tf1;
            ws.offx = (int) wot;                         // receive(): ONE block, the ADC's window (integrator.cpp:624-628)
            ws.offy = (int) wof;
            ws.bw = ws.W = (int) lp.bins;
            ws.bh = ws.H = (int) lp.bins_y;
            ws.cropx = (int) wot;
            ws.cropy = (int) wof;
            ws.C = 3u + P + (mom ? (lp.iq ? 2u : 1u) : 0u);
            ws.m2off = ws.nch = 0u;
            ws.qch = 3u + P;
            ws.q2 = lp.iq != 0u;
            ws.v0 = a0;
            ws.v1 = a1;
            ws.v2 = 1.f;
            ws.v3 = ws.v4 = 0.f;
            ws.five = false;
            ws.ech = 3 + pk0 - 1;
            ws.emask = pmask;
            ws.e3 = false;
            ws.e0 = pv;
            ws.e1 = ws.e2 = 0.f;
            put_wide<mom, sum>(se, ws, hd);
        } else {
            ++acc.invalid;
        }
    } else if ((ok = ok && lx >= 0.f && lx < (float) lp.bins && ly >= 0.f && ly < (float) lp.bins_y)) {
        uint32_t off = (3u + P + (mom ? (lp.iq ? 2u : 1u) : 0u)) * ((uint32_t) ly * lp.bins + (uint32_t) lx);
        if (a0 != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, off + 0u, a0);
        if (a1 != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, off + 1u, a1);
        hist_add<sum>(s_hist, g_hist, lds_hist, off + 2u, 1.f);
        if (mom) {
            if (q0 != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, off + 3u + P, q0);
            if (lp.iq && q1 != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, off + 4u, q1);
        }
        for (int i = 0; i < 3; ++i)
            if ((pmask >> i & 1u) && pv != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, off + 3u + (uint32_t) (pk0 - 1 + i), pv);
        acc.W += 1.f;
    } else {
        ++acc.invalid;
    }
    rec_L = a0;
    rec_aux = lp.iq ? a1 : s.t_rx - se.adc_sampling_start;
}

// bf_path_record {L, aux, valid, n_rays} of a path whose sample has been put
BF_DEV void record_put(const DLaunch &lp, const PathState &s, bf_path_record *records, float rec_L, float rec_aux, bool valid) {
    uint64_t rec_i = s.path_i;
    if (lp.roll) {              // rolling sequence: the render's own record array, indexed by the local path
        records = lp.has_records ? lp.roll[s.render & (kRollRing - 1u)].records : nullptr;     // (no per-path fetch of a null pointer)
        rec_i -= (uint64_t) s.render * lp.batch_paths;
    }
    if (records) {
        // bf_path_record {L, aux, valid, n_rays} as one 16-byte store through a global-address-space pointer (a rolling render's
        // array comes out of its descriptor: a generic pointer would make this a flat store)
        static_assert(sizeof(bf_path_record) == 16, "one 16-byte store per record");
        typedef __attribute__((address_space(1))) bf_f4 *glb_f4_ptr;
        bf_f4 r;
        r.x = rec_L;
        r.y = rec_aux;
        r.z = __uint_as_float(valid ? 1u : 0u);
        r.w = __uint_as_float(s.n_rays);
        ((glb_f4_ptr) records)[rec_i] = r;
    }
}

// render_sample / receive_sample tail: the sample of a finished path into its render's histogram, the path into the records.
// The render modes' ImageBlock::put, with the range / time AOVs, stands here; the receive modes' SignalBlock::put is film_put_receive
template <int RX = 2>
BF_DEV void film_put(const DScene &sc0, const DLaunch &lp, const PathState &s, float *s_hist, float *g_hist, bool lds_hist,
                     FilmAcc &acc, bf_path_record *records, const AovCtx &av = aov_none()) {
    const DScene sc = path_scene<RX>(sc0, lp, s.render);
    const bool valid = (s.flags & kFlagValid) != 0;
    ++acc.n_put;
    float rec_L, rec_aux;
    constexpr bool aov = (RX & kAov) != 0;         // BF_FLAG_AOV: the first intersection's AOVs behind the base channels, nested.RGBA last
    float *const s_base = s_hist + (aov ? 0u : lp.base_off);                  // rolling launches: base-channel table (DLaunch::base_off; an AOV launch keeps its table word there)
    constexpr bool classed = (RX & kClass) != 0;   // BF_FLAG_CLASSES: one histogram block per class of the path's first intersection
    // this render's block of the histogram (classed: the block of the path's class within it)
    const uint32_t n_cls = classed ? scene_n_classes(sc0) : 0u;
    constexpr bool sum = (RX & kSum) != 0;         // BF_FLAG_EXACT_SUM: the cells are limbs (hist_add), s_hist and g_hist limb arrays
    const HistDst hd = hist_dst<sum>(lp, s.render, s_hist, g_hist, lds_hist, n_cls, classed ? s.cls : 0u);
    s_hist = hd.s;
    g_hist = hd.g;
    lds_hist = hd.lds;
    if (mode_receive<RX>(lp)) {
        film_put_receive<RX>(sc, lp, s, hd, valid, acc, rec_L, rec_aux);
    } else {
        constexpr bool wide = (RX & kWide) != 0;       // reconstruction filter wider than a pixel (uniform; the radar scenes use box)
        constexpr bool mom = (RX & kMoment) != 0;      // BF_FLAG_MOMENT: second moments next to every first-moment channel (beifong_hip.h)
        const bool is_range = lp.mode == BF_MODE_RANGE, is_time = rare<RX>(lp.mode == BF_MODE_TIME);
        // ray weight: fluxmeter.cpp:84 (wav_weight * pi), irradiancemeter.cpp:82 (wav_weight * pi / surface_area),
        // perspective.cpp:198 (wav_weight)
        float sensor_w = 1.f;
        if (rare<RX>(c_sensor(sc).type == BF_SENSOR_FLUXMETER)) sensor_w = 1.f * kPi;
        if (rare<RX>(c_sensor(sc).type == BF_SENSOR_IRRADIANCEMETER)) sensor_w = 1.f * kPi / c_rects(sc)[c_sensor(sc).rect].area;
        float L = sensor_w * s.result;                        // integrator.cpp:286
        float X, Y, Z;
        if (lp.color_mode == BF_COLOR_RGB)
            srgb_to_xyz_grey(L, X, Y, Z);
        else
            X = Y = Z = L;
        float a0 = s.result, a1 = s.result, a2 = s.result;    // AOVs see the unweighted radiance
        if (is_time && lp.color_mode == BF_COLOR_RGB) srgb_to_xyz_grey(s.result, a0, a1, a2);
        bool ok = (s.flags & kFlagFilmOk) && __builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z);
        if (is_range || is_time) ok = ok && __builtin_isfinite(a0) && __builtin_isfinite(a1) && __builtin_isfinite(a2);
        // aov.cpp:170-251: per pixel X Y Z A W | the table's K floats | nested AOVs from channel eb | nested.R G B A at rch.  The values wait
        // in the slot's side rows since the first vertex; one of them that is not finite drops the sample like any other channel
        const uint32_t eb = 5u + (aov ? av.K : 0u);
        AovVals avv;
        bool afin = true;
        if (aov) {
            avv = aov_load(av);
                afin = __builtin_isfinite(s.result) && __builtin_isfinite(avv.t) && __builtin_isfinite(avv.px) && __builtin_isfinite(avv.py) &&
                       __builtin_isfinite(avv.pz) && __builtin_isfinite(avv.u) && __builtin_isfinite(avv.v) && __builtin_isfinite(avv.nx) &&
                       __builtin_isfinite(avv.ny) && __builtin_isfinite(avv.nz) && __builtin_isfinite(avv.sx) && __builtin_isfinite(avv.sy) &&
                       __builtin_isfinite(avv.sz) && __builtin_isfinite(avv.ux) && __builtin_isfinite(avv.uy) && __builtin_isfinite(avv.uz) &&
                       __builtin_isfinite(avv.vx) && __builtin_isfinite(avv.vy) && __builtin_isfinite(avv.vz);
            ok = ok && afin;
        }
        // moment.cpp:72-91: nested.XYZ = the XYZ of the nested (unweighted) result, then the square of every nested channel.
        // A nested AOVs; per pixel: X Y Z A W | AOVs | nested.XYZ at nch | m2_ AOVs (m2off behind each) | m2_ nested.XYZ at qch
        const uint32_t n_aov = is_range ? lp.bins : (is_time ? 3u * lp.bins : 0u);
            const uint32_t nch = 5u + n_aov, m2off = n_aov + 3u, qch = 8u + 2u * n_aov;
        float nX = 0.f, nY = 0.f, nZ = 0.f, qX = 0.f, qY = 0.f, qZ = 0.f;
        bool mfin = true;
        if (mom) {
            if (lp.color_mode == BF_COLOR_RGB)
                srgb_to_xyz_grey(s.result, nX, nY, nZ);
            else
                nX = nY = nZ = s.result;
            qX = nX * nX;
            qY = nY * nY;
            qZ = nZ * nZ;
            // ImageBlock::put refuses a sample with ANY non-finite channel: also one whose square overflows
            mfin = __builtin_isfinite(nX) && __builtin_isfinite(nY) && __builtin_isfinite(nZ) && __builtin_isfinite(qX) &&
                   __builtin_isfinite(qY) && __builtin_isfinite(qZ);
            if (is_range || is_time) mfin = mfin && __builtin_isfinite(a0 * a0) && __builtin_isfinite(a1 * a1) && __builtin_isfinite(a2 * a2);
            ok = ok && mfin;
        }
        // multi-pixel film: every channel of the sample goes to its pixel's block of the histogram; the 1 x 1 film
        // keeps the five base channels in registers until film_flush
        uint32_t pix = 0u;
        // the five base channels of a 1 x 1 film are summed in registers while every lane of the wave feeds the same
        // histogram: a plain launch, or the newest render of a rolling sequence.  Never in a class launch: the lanes' paths belong to
        // different class blocks, so the base channels go cell by cell like a W x H film's (the class is one more film axis)
        // Nor in an exact-sum launch: a register sum is an fp32 sum in lane order
        const bool use_acc = !classed && !sum && (lp.batch == 0u || (lp.roll != nullptr && s.render == lp.roll_newest));
        if (rare<RX>(lp.spp != 0u)) {
            const uint64_t q = (lp.path_offset + s.path_i) / lp.spp;
            const uint32_t px = (uint32_t) (q % lp.film_w) - ((s.flags & kFlagFilmLeft) ? 1u : 0u);
            const uint32_t py = (uint32_t) (q / lp.film_w) - ((s.flags & kFlagFilmUp) ? 1u : 0u);
            pix = (py * lp.film_w + px) * lp.chan_px;          // only used when kFlagFilmOk
        }
        if (wide) {
            // the filtered branch takes every finite sample (where it lands is decided cell by cell)
            bool fin = __builtin_isfinite(X) && __builtin_isfinite(Y) && __builtin_isfinite(Z);
            if (is_range || is_time) fin = fin && __builtin_isfinite(a0) && __builtin_isfinite(a1) && __builtin_isfinite(a2);
            if (mom) fin = fin && mfin;
            if (aov) fin = fin && afin;
            if (fin) {
                WideSample ws;
                uint32_t qx, qy;
                float fx, fy;
                film_position(lp, s, qx, qy, fx, fy);
                ws.cropx = (int) c_sensor(sc).crop_x;         // blocks tile the crop window from its offset (spiral.cpp: offset += m_offset)
                ws.cropy = (int) c_sensor(sc).crop_y;
                ws.posx = (float) (qx + (uint32_t) ws.cropx) + fx;
                ws.posy = (float) (qy + (uint32_t) ws.cropy) + fy;
                const uint32_t B = c_sensor(sc).filt_block;
                const int bx0 = B ? (int) (qx / B * B) : 0, by0 = B ? (int) (qy / B * B) : 0;
                ws.offx = ws.cropx + bx0;
                ws.offy = ws.cropy + by0;
                ws.W = (int) lp.film_w;
                ws.H = (int) lp.film_h;
                ws.bw = B ? min((int) B, ws.W - bx0) : ws.W;
                ws.bh = B ? min((int) B, ws.H - by0) : ws.H;
                ws.C = lp.chan_px;
                ws.v0 = X;
                ws.v1 = Y;
                ws.v2 = Z;
                ws.v3 = valid ? 1.f : 0.f;
                ws.v4 = 1.f;
                ws.five = true;
                ws.emask = 0u;
                ws.e3 = is_time;
                ws.ech = (int) eb;
                ws.e0 = a0;
                ws.e1 = a1;
                ws.e2 = a2;
                ws.m2off = m2off;
                ws.nch = nch;
                ws.qch = qch;
                ws.n0 = nX;
                ws.n1 = nY;
                ws.n2 = nZ;
                ws.q2 = false;
                if (is_range || is_time) {
                    float w = lp.bin_width;
                    int k = (int) __builtin_floorf(s.aux / w);
                    ws.ech = (int) eb + (k - 1) * (is_time ? 3 : 1);
                    for (int i = k - 1; i <= k + 1; ++i) {
                        if (i < 0 || i >= (int) lp.bins) continue;
                        float lo = (float) i * w, hi = (float) i * w + w;
                        if (s.aux >= lo && s.aux < hi) ws.emask |= 1u << (i - (k - 1));
                    }
                }
                put_wide<mom, sum>(c_sensor(sc), ws, hd);
                if (aov) put_wide_aov(c_sensor(sc), ws, hd, av, avv, eb + n_aov, s.result, valid ? 1.f : 0.f);
            } else {
                ++acc.invalid;
            }
        } else if (ok) {
            if (rare<RX>(lp.spp != 0u)) {
                    if (X != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + 0u, X);
                    if (Y != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + 1u, Y);
                    if (Z != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + 2u, Z);
                    if (valid) hist_add<sum>(s_hist, g_hist, lds_hist, pix + 3u, 1.f);
                    hist_add<sum>(s_hist, g_hist, lds_hist, pix + 4u, 1.f);
                    if (mom) {
                        if (nX != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + nch + 0u, nX);
                        if (nY != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + nch + 1u, nY);
                        if (nZ != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + nch + 2u, nZ);
                        if (qX != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + qch + 0u, qX);
                        if (qY != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + qch + 1u, qY);
                        if (qZ != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + qch + 2u, qZ);
                    }
            } else if (!use_acc) {
                // batched launch: the wave's lanes hold paths of different renders, so the base channels cannot be
                // summed in registers; each sample goes to its render's block.  A rolling sequence's older renders (behind
                // the LDS window) would hit the same five GLOBAL addresses from every wave: they go through the
                // workgroup's base-channel table instead (kRollBase renders; film_flush adds it up)
                float *bs = s_hist;
                bool bl = lds_hist;
                uint32_t bn = nch, bq = qch;       // kMoment: where nested.XYZ and their squares go (the table keeps its eleven entries together)
                // a class launch too large for an LDS histogram: every wave would hit the same five GLOBAL addresses per class, so
                // the base channels go through the workgroup's class table [render][class][5] (DLaunch::lds_floats; film_flush adds it up)
                if (classed && !lds_hist && lp.lds_floats != 0u) {
                    bs = s_base + kRollBaseCh * ((lp.batch != 0u ? s.render * n_cls : 0u) + s.cls);
                    bl = true;
                }
                // likewise an exact-sum launch too large for LDS limbs: the workgroup's table [render][5] of limb cells
                if (sum && !lds_hist && lp.lds_floats != 0u) {
                    bs = s_base + (uint32_t) bfs::kCellFloats * kRollBaseCh * (lp.batch != 0u ? s.render : 0u);
                    bl = true;
                }
                if (lp.roll && !lds_hist && lp.roll_newest - s.render < kRollBase) {
                    bs = s_base + (mom ? kRollBaseChMoment : kRollBaseCh) * (lp.roll_newest - s.render);
                    bl = true;
                    bn = 5u;
                    bq = 8u;
                }
                    if (X != 0.f) hist_add<sum>(bs, g_hist, bl, 0u, X);
                    if (Y != 0.f) hist_add<sum>(bs, g_hist, bl, 1u, Y);
                    if (Z != 0.f) hist_add<sum>(bs, g_hist, bl, 2u, Z);
                    if (valid) hist_add<sum>(bs, g_hist, bl, 3u, 1.f);
                    hist_add<sum>(bs, g_hist, bl, 4u, 1.f);
                    if (mom) {
                        if (nX != 0.f) hist_add<sum>(bs, g_hist, bl, bn + 0u, nX);
                        if (nY != 0.f) hist_add<sum>(bs, g_hist, bl, bn + 1u, nY);
                        if (nZ != 0.f) hist_add<sum>(bs, g_hist, bl, bn + 2u, nZ);
                        if (qX != 0.f) hist_add<sum>(bs, g_hist, bl, bq + 0u, qX);
                        if (qY != 0.f) hist_add<sum>(bs, g_hist, bl, bq + 1u, qY);
                        if (qZ != 0.f) hist_add<sum>(bs, g_hist, bl, bq + 2u, qZ);
                    }
            } else {
                acc.X += X;
                acc.Y += Y;
                acc.Z += Z;
                acc.A += valid ? 1.f : 0.f;
                acc.W += 1.f;
                if (mom) {
                    acc.nX += nX;
                    acc.nY += nY;
                    acc.nZ += nZ;
                    acc.qX += qX;
                    acc.qY += qY;
                    acc.qZ += qZ;
                }
            }
                if (aov) {
                    // box filter: the value itself (a 1 x 1 film's paths all feed the same K + 4 cells, like the bins below)
                    uint32_t ch = pix + 5u;
                    for (uint64_t t = av.types; t & 15u; t >>= 4) {
                        const uint32_t type = (uint32_t) (t & 15u) - 1u, nf = aov_type_floats(type);
                        float vx, vy, vz;
                        aov_entry(avv, type, vx, vy, vz);
                        if (vx != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, ch, vx);
                        if (nf > 1u && vy != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, ch + 1u, vy);
                        if (nf > 2u && vz != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, ch + 2u, vz);
                        ch += nf;
                    }
                    const uint32_t rch = pix + eb + n_aov;
                    if (s.result != 0.f) {
                        hist_add<sum>(s_hist, g_hist, lds_hist, rch + 0u, s.result);
                        hist_add<sum>(s_hist, g_hist, lds_hist, rch + 1u, s.result);
                        hist_add<sum>(s_hist, g_hist, lds_hist, rch + 2u, s.result);
                    }
                    if (valid) hist_add<sum>(s_hist, g_hist, lds_hist, rch + 3u, 1.f);
                }
            if (is_range || is_time) {
                // range.cpp:141-161 / time.cpp:134-153: bin i takes the sample iff
                // (float)i*w <= aux < (float)i*w + w, evaluated exactly as written
                // there for the (at most three) candidate bins
                float w = lp.bin_width;
                int k = (int) __builtin_floorf(s.aux / w);
                for (int i = k - 1; i <= k + 1; ++i) {
                    if (i < 0 || i >= (int) lp.bins) continue;
                    float lo = (float) i * w, hi = (float) i * w + w;
                    if (s.aux >= lo && s.aux < hi) {
                        if (is_range) {
                            if (a0 != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + eb + (uint32_t) i, a0);
                            if (mom && a0 != 0.f) hist_add<sum>(s_hist, g_hist, lds_hist, pix + eb + (uint32_t) i + m2off, a0 * a0);
                        } else if (a0 != 0.f || a1 != 0.f || a2 != 0.f) {
                            hist_add<sum>(s_hist, g_hist, lds_hist, pix + eb + 3u * (uint32_t) i + 0u, a0);
                            hist_add<sum>(s_hist, g_hist, lds_hist, pix + eb + 3u * (uint32_t) i + 1u, a1);
                            hist_add<sum>(s_hist, g_hist, lds_hist, pix + eb + 3u * (uint32_t) i + 2u, a2);
                            if (mom) {
                                hist_add<sum>(s_hist, g_hist, lds_hist, pix + eb + 3u * (uint32_t) i + m2off + 0u, a0 * a0);
                                hist_add<sum>(s_hist, g_hist, lds_hist, pix + eb + 3u * (uint32_t) i + m2off + 1u, a1 * a1);
                                hist_add<sum>(s_hist, g_hist, lds_hist, pix + eb + 3u * (uint32_t) i + m2off + 2u, a2 * a2);
                            }
                        }
                    }
                }
            }
        } else {
            ++acc.invalid;
        }
        rec_L = L;
        rec_aux = s.aux;
    }
    record_put(lp, s, records, rec_L, rec_aux, valid);
}

// film_flush, render modes: wave-reduce the base channels a 1 x 1 film's lanes kept in registers; lane 0 adds them to the histogram
template <int RX> BF_DEV void flush_wave_acc(const DLaunch &lp, FilmAcc &acc, float *s_hist, float *g_hist, bool lds_hist, int lane) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc.X += __shfl_down(acc.X, off);
        acc.Y += __shfl_down(acc.Y, off);
        acc.Z += __shfl_down(acc.Z, off);
        acc.A += __shfl_down(acc.A, off);
        acc.W += __shfl_down(acc.W, off);
        if (RX & kMoment) {
            acc.nX += __shfl_down(acc.nX, off);
            acc.nY += __shfl_down(acc.nY, off);
            acc.nZ += __shfl_down(acc.nZ, off);
            acc.qX += __shfl_down(acc.qX, off);
            acc.qY += __shfl_down(acc.qY, off);
            acc.qZ += __shfl_down(acc.qZ, off);
        }
    }
    // (kClass: film_put has written the base channels already, acc.W is 0)
    if (lane == 0 && acc.W != 0.f && !lp.spp && (lp.batch == 0u || lp.roll != nullptr)) {
        const HistDst hd = hist_dst(lp, lp.roll ? lp.roll_newest : 0u, s_hist, g_hist, lds_hist);
        hist_add(hd.s, hd.g, hd.lds, 0, acc.X);
        hist_add(hd.s, hd.g, hd.lds, 1, acc.Y);
        hist_add(hd.s, hd.g, hd.lds, 2, acc.Z);
        hist_add(hd.s, hd.g, hd.lds, 3, acc.A);
        hist_add(hd.s, hd.g, hd.lds, 4, acc.W);
        if (RX & kMoment) {
                // the 1 x 1 film: chan_px = 5 + 2 (A + 3) channels; nested.XYZ behind the A nested AOVs, their squares last
                const uint32_t nch = (lp.chan_px - 1u) / 2u, qch = lp.chan_px - 3u;
            if (acc.nX != 0.f) hist_add(hd.s, hd.g, hd.lds, nch + 0u, acc.nX);
            if (acc.nY != 0.f) hist_add(hd.s, hd.g, hd.lds, nch + 1u, acc.nY);
            if (acc.nZ != 0.f) hist_add(hd.s, hd.g, hd.lds, nch + 2u, acc.nZ);
            if (acc.qX != 0.f) hist_add(hd.s, hd.g, hd.lds, qch + 0u, acc.qX);
            if (acc.qY != 0.f) hist_add(hd.s, hd.g, hd.lds, qch + 1u, acc.qY);
            if (acc.qZ != 0.f) hist_add(hd.s, hd.g, hd.lds, qch + 2u, acc.qZ);
        }
    }
}
// kSum: n_cells limb cells of LDS into the same cells of global memory, one global atomic per non-zero limb
BF_DEV void flush_limbs(float *s_limbs, float *g_limbs, uint32_t n_cells, int tid) {
    __syncthreads();
    const lds_i64_ptr s = (lds_i64_ptr) reinterpret_cast<long long *>(s_limbs);
    long long *const g = reinterpret_cast<long long *>(g_limbs);
    for (uint32_t i = tid; i < n_cells * (uint32_t) bfs::kLimbs; i += kBlock) {
        const long long v = s[i];
        if (v != 0) glb_add_i64(g + i, v);
    }
}
// film_flush: the LDS-privatised histogram, one global atomic per non-empty bin
template <bool SUM = false> BF_DEV void flush_lds_hist(const DLaunch &lp, float *s_hist, float *g_hist, int tid) {
    if (SUM) {      // (never rolling)
        flush_limbs(s_hist, g_hist, lp.n_chan_all, tid);
        return;
    }
    __syncthreads();
    if (lp.roll) {
        // one block per render of the LDS window, each flushed into that render's own histogram
        for (uint32_t r = lp.roll_lo; r <= lp.roll_newest; ++r) {
            float *gh = lp.roll[r & (kRollRing - 1u)].hist;
            const float *sh = s_hist + (r - lp.roll_lo) * lp.n_chan;
            for (uint32_t i = tid; i < lp.n_chan; i += kBlock) {
                float v = sh[i];
                if (v != 0.f) glb_add(gh + i, v);
            }
        }
    } else {
        for (uint32_t i = tid; i < lp.n_chan_all; i += kBlock) {
            float v = s_hist[i];
            if (v != 0.f) glb_add(g_hist + i, v);
        }
    }
}
// film_flush: the class table of a launch without an LDS histogram (film_put): entry [render][class][channel] -> the block's
// base channels
BF_DEV void flush_class_table(const DLaunch &lp, float *s_hist, float *g_hist, int tid) {
    __syncthreads();
    for (uint32_t i = tid; i < lp.lds_floats; i += kBlock) {
        const float v = s_hist[i];
        const uint32_t blk = i / kRollBaseCh;
        if (v != 0.f) glb_add(g_hist + (size_t) blk * lp.n_chan + (i - kRollBaseCh * blk), v);
    }
}
// film_flush: the base-channel table of an exact-sum launch without LDS limbs (film_put): limb [render][channel][limb] -> the same limb
// of the render's base cells
BF_DEV void flush_sum_table(const DLaunch &lp, float *s_hist, float *g_hist, int tid) {
    __syncthreads();
    const lds_i64_ptr s = (lds_i64_ptr) reinterpret_cast<long long *>(s_hist);
    long long *const g = reinterpret_cast<long long *>(g_hist);
    for (uint32_t i = tid; i < lp.lds_floats / 2u; i += kBlock) {
        const long long v = s[i];
        const uint32_t cell = i / (uint32_t) bfs::kLimbs, render = cell / kRollBaseCh;
        if (v != 0) glb_add_i64(g + ((size_t) render * lp.n_chan + (cell - kRollBaseCh * render)) * bfs::kLimbs + (i - (uint32_t) bfs::kLimbs * cell), v);
    }
}
// film_flush: the base-channel table of the renders behind the window: entry [age][channel], age = roll_newest - render
template <int RX> BF_DEV void flush_roll_base(const DLaunch &lp, float *s_hist, bool lds_hist, int tid) {
    if (!lds_hist) __syncthreads();
    const float *s_base = s_hist + lp.base_off;
    constexpr uint32_t kB = (RX & kMoment) ? kRollBaseChMoment : kRollBaseCh;
    for (uint32_t i = tid; i < kB * kRollBase; i += kBlock) {
        const float v = s_base[i];
        const uint32_t age = i / kB;
        uint32_t ch = i - kB * age;
        // moment sequences: entries 5-7 are nested.XYZ, 8-10 their squares (film_put): back to their channels of the 1 x 1 film
        if ((RX & kMoment) && ch >= 5u) ch = ch < 8u ? (lp.chan_px - 1u) / 2u + (ch - 5u) : lp.chan_px - 3u + (ch - 8u);
        if (v != 0.f && age <= lp.roll_newest) glb_add(lp.roll[(lp.roll_newest - age) & (kRollRing - 1u)].hist + ch, v);
    }
}

// wave-reduce the base channels into the histogram (render modes only) and
// flush the LDS-privatised histogram: one global atomic per non-empty bin
template <int RX = 2> BF_DEV void film_flush(const DLaunch &lp, FilmAcc &acc, float *s_hist, float *g_hist, bool lds_hist, int tid) {
    const int lane = tid & 63;
    // (kSum: film_put has written the base channels as limbs, no lane holds a register sum)
    if (!(RX & kSum) && !mode_receive<RX>(lp)) flush_wave_acc<RX>(lp, acc, s_hist, g_hist, lds_hist, lane);
    if (lds_hist) flush_lds_hist<(RX & kSum) != 0>(lp, s_hist, g_hist, tid);
    if ((RX & kClass) && !lds_hist && lp.lds_floats != 0u) flush_class_table(lp, s_hist, g_hist, tid);
    if ((RX & kSum) && !lds_hist && lp.lds_floats != 0u) flush_sum_table(lp, s_hist, g_hist, tid);
    if (lp.roll && !mode_receive<RX>(lp)) flush_roll_base<RX>(lp, s_hist, lds_hist, tid);
}

BF_NS_END  // namespace bfd
