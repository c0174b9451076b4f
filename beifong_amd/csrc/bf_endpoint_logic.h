// The transmitter / receiver plugin arithmetic of the receive modes, called by generate_path, shade_vertex (bf_path_logic.h) and
// film_put (bf_film.h):
//
//   jabs ... wchirp_j, phase_update : the "Jacob functions" (math.h:62-131) and Ray::update_state's phase (ray.h:89-93)
//   rect_sample_wigner              : Rectangle::sample_wigner (rectangle.cpp:132-220)
//   phased_sample_wigner            : phasedtransmitter.cpp:273-291, phasedreceiver.cpp:279-297
//   tx_* , transmitter_*            : areatransmitter.cpp:65-186, wignertransmitter.cpp:111-577, phasedtransmitter.cpp:296-620
//   receiver_sample_ray             : omnidirectional.cpp:72-107, wignerreceiver.cpp:118-269, phasedreceiver.cpp:299-365
#pragma once
#include "bf_device_core.h"

BF_NS_BEGIN

// ---------------------------------------------------------------------------
// gen-3 building blocks: "Jacob functions" (math.h:62-131), the rectangular
// aperture Wigner gain (rectangle.cpp:132-220), the transmitter signal model
// (wignertransmitter.cpp:111-146).  A literal `1e-9` is a double in the
// reference, so those products run in double here too.
// ---------------------------------------------------------------------------
BF_DEV float jabs(float x) { return x >= 0.f ? x : -x; }
// Ray::update_state, phase part (ray.h:89-93): float product, double quotient and sum, float store;
// the divisor is HALF THE BAND WIDTH in metres (Q4)
BF_DEV float phase_update(float phase, float t, float lambda_min_nm, float lambda_max_nm) {
    float num = 6.28318530717958647692f * t;
    double den = (double) ((lambda_max_nm - lambda_min_nm) / 2.f) * 1e-9;
    return (float) ((double) phase + (double) num / den);
}
BF_DEV float sinc_j(float x) { return jabs(x) > kEpsilon ? sin_cr(x) / x : 1.f; }
BF_DEV float tri_j(float x) { return jabs(x) < 0.5f ? 1.f - 2.f * jabs(x) : 0.f; }
BF_DEV float rect_j(float x) { return jabs(x) < 0.5f ? 1.f : 0.f; }
BF_DEV float fmodulo_j(float a, float b) {
    float result = jabs(a);
    int guard = 0;
    while (result - jabs(b) >= kEpsilon && guard++ < (1 << 22)) result -= jabs(b);
    result = (a < 0.f) ? jabs(b) - result : result;
    result += (b < 0.f) ? b : 0.f;
    return result;
}
BF_DEV float wchirp_j(float t, float f, float w, float a) {
    return 2 * a * a * w * tri_j(t / w) * sinc_j(6.28318530717958647692f * f * w * tri_j(t / w));
}
BF_DEV float rect_sample_wigner(CRect &rc, V3 p, V3 d, float lambda_nm) {
    const float kTwoPi = 6.28318530717958647692f;
    V3 fs = mk(rc.s[0], rc.s[1], rc.s[2]), ft = mk(rc.t[0], rc.t[1], rc.t[2]), fn = mk(rc.n[0], rc.n[1], rc.n[2]);
    float wid_x = norm(fs), wid_y = norm(ft);
    V3 r_hat = xf_point(rc.to_object, p) / 2.f;
    V3 ns = normalize(fs), nt = normalize(ft);
    (void) fn;
    float lx = dot(ns, d), ly = dot(nt, d);
    double inv = 1.0 / ((double) lambda_nm * 1e-9);
    float nu_x = (float) ((double) lx * inv), nu_y = (float) ((double) ly * inv);
    return 4 * tri_j(r_hat.x) * tri_j(r_hat.y) * sinc_j(kTwoPi * nu_x * wid_x * tri_j(r_hat.x)) *
           sinc_j(kTwoPi * nu_y * wid_y * tri_j(r_hat.y));
}
// PhasedTransmitter / Phasedreceiver::sample_wigner — phasedtransmitter.cpp:273-291, phasedreceiver.cpp:279-297:
// real part of the sum over the n^2 virtual elements of
//   W_rect_2D(r, nu, wid) * exp(j 2 pi nu . r') * psi',   r = velem_to_object * p / 2 (only |r.x|, |r.y| <= 0.5),
//   nu = dir_to_local * d / (lambda 1e-9)
template <class W> BF_DEV float phased_sample_wigner(const float *__restrict__ tab, uint32_t n, W wid, V3 p, V3 d, float lambda_nm) {
    const float kTwoPi = 6.28318530717958647692f;
    const double inv = 1.0 / ((double) lambda_nm * 1e-9);
    float w_re = 0.f;
    for (uint32_t i = 0; i < n; ++i) {
        const float *e = tab + (size_t) BF_VELEM_FLOATS * i;
        V3 r_hat = xf_point(e, p) / 2.f;
        if (jabs(r_hat.x) <= 0.5f && jabs(r_hat.y) <= 0.5f) {
            V3 md = xf_vector(e + 12, d);
            V3 nu = mk((float) ((double) md.x * inv), (float) ((double) md.y * inv), (float) ((double) md.z * inv));
            float tx = tri_j(r_hat.x), ty = tri_j(r_hat.y);
            float wr = 4 * wid[0] * wid[1] * tx * ty * sinc_j(kTwoPi * nu.x * wid[0] * tx) * sinc_j(kTwoPi * nu.y * wid[1] * ty);
            float sn, cs;
            bf_sincos(kTwoPi * dot(nu, mk(e[24], e[25], e[26])), sn, cs);
            float a = wr * cs, b = wr * sn;                       // W_rect * exp(j ...)
            w_re += a * e[28] - b * e[29];                        // ... * psi', real part
        }
    }
    return w_re;
}
BF_DEV float tx_eval_signal(CEmitter &e, float time, float frequency) {
    if (e.signal_type == BF_SIGNAL_LINFMCW) {
        float t = fmodulo_j(time, rcp_ieee(e.prf));
        float ti = 0 + e.pulse_len / 2;
        float fi = e.freq_centre + div_ieee(e.freq_ext, e.pulse_len) * (t - ti);
        return rect_j((t - ti) / e.pulse_len) > 0.f ? wchirp_j(t - ti, frequency - fi, e.pulse_len, e.amplitude) : 0.f;
    } else if (e.signal_type == BF_SIGNAL_PULSE) {
        float t = fmodulo_j(time, rcp_ieee(e.prf));
        float ti = 0 + e.pulse_len / 2;
        float fi = e.freq_centre;
        return rect_j((t - ti) / e.pulse_len) > 0.f ? wchirp_j(t - ti, frequency - fi, e.pulse_len, e.amplitude) : 0.f;
    }
    return e.amplitude * e.amplitude;
}
BF_DEV float freq_of(float c, float lambda_nm) { return (float) ((double) c * (1.0 / ((double) lambda_nm * 1e-9))); }
// WignerTransmitter::sample_delta_frequency (wignertransmitter.cpp:152-168), the frequency only: the instantaneous frequency of the
// chirp ("linfmcw") or the carrier ("cw") at `time`; the weight it returns is 1 whatever eval_signal says (:165).  "pulse" leaves
// `frequencies` uninitialised there: refused at scene creation (bf_api.cpp).
BF_DEV float tx_delta_frequency(CEmitter &e, float time) {
    if (e.signal_type == BF_SIGNAL_LINFMCW) {
        float t = fmodulo_j(time, rcp_ieee(e.prf));
        float ti = 0 + e.pulse_len / 2;
        return e.freq_centre + div_ieee(e.freq_ext, e.pulse_len) * (t - ti);
    }
    return e.freq_centre;
}
// m_resample_freq (wignertransmitter.cpp:211-221, 430-441; phasedtransmitter.cpp likewise): the interaction's wavelength is
// overwritten with MTS_C * rcp(frequency) * 1e9 (a double product rounded to Float) before anything else reads it, and the signal
// power is 1
BF_DEV float tx_resampled_lambda(const DScene &sc, CEmitter &e, float time) {
    return (float) ((double) (sc.c * rcp_ieee(tx_delta_frequency(e, time))) * 1e9);
}

// Transmitter::eval — areatransmitter.cpp:65-73, wignertransmitter.cpp:193-271
template <int V = 0> BF_DEV float transmitter_eval(const DScene &sc, CEmitter &e, const SI &si, float si_time, float &lambda0) {
    CRect &rc = c_rects(sc)[e.rect];
    if (e.type == BF_TRANSMITTER_AREA) return (si.wi.z > 0.f) ? e.radiance * rc.area : 0.f;
    float signal_power;
    if (rare<V>(e.resample != 0u)) {
        lambda0 = tx_resampled_lambda(sc, e, si_time);           // si.wavelengths = ... (the path carries it on: spawn_ray, :451)
        signal_power = 1.f;
    } else {
        signal_power = tx_eval_signal(e, si_time, freq_of(sc.c, lambda0));
    }
    if (rare<V>(e.type == BF_TRANSMITTER_PHASED)) {
        // phasedtransmitter.cpp:296-381: geom_gain = antenna / area * sample_wigner(ds with the uninitialised d, Q5)
        float geom_gain = 1.f * rcp(rc.area);
        geom_gain *= phased_sample_wigner(e.velems, e.n_velems, e.wid, si.p, mk(-0.f, -0.f, -0.f), lambda0);
        return (si.wi.z > 0.f) ? signal_power * e.gain * geom_gain : 0.f;
    }
    float ws = rect_sample_wigner(rc, si.p, mk(0.f, 0.f, 0.f), lambda0);   // Q5: ds.d never initialised -> 0
    return (si.wi.z > 0.f) ? signal_power * e.gain * (1.f * ws) * 6.28318530717958647692f : 0.f;
}
// Transmitter::sample_direction — areatransmitter.cpp:117-165, wignertransmitter.cpp:373-534
template <int V = 0>
BF_DEV float transmitter_sample_direction(const DScene &sc, CEmitter &e, V3 ref_p, float ref_time, float &lambda0,
                                          float sx, float sy, DirSample &ds) {
    CRect &rc = c_rects(sc)[e.rect];
    V3 p = xf_point(rc.to_world, mk(sx * 2.f - 1.f, sy * 2.f - 1.f, 0.f));
    V3 n = mk(rc.n[0], rc.n[1], rc.n[2]);
    ds.pdf = rc.inv_area;
    ds.delta = false;
    ds.d = p - ref_p;
    float dist_squared = squared_norm(ds.d);
    ds.dist = __builtin_sqrtf(dist_squared);
    ds.d = ds.d / ds.dist;
    float dp = __builtin_fabsf(dot(ds.d, n));
    ds.pdf *= (dp != 0.f) ? dist_squared / dp : 0.f;
    bool active = dot(ds.d, n) < 0.f && ds.pdf != 0.f;
    if (e.type == BF_TRANSMITTER_AREA) {
        float spec = e.radiance / ds.pdf;
        return active ? spec : 0.f;
    }
    float geom_gain = 1.f / ds.pdf;
    float t = ref_time;
    if ((double) ds.dist > 5e-7) t += -ds.dist / sc.c;                      // retarded time :422-425
    float signal_power;
    if (rare<V>(e.resample != 0u)) {
        lambda0 = tx_resampled_lambda(sc, e, t);                 // it.wavelengths = ... : whether or not the sample is used
        signal_power = 1.f;
    } else {
        signal_power = tx_eval_signal(e, t, freq_of(sc.c, lambda0));
    }
    if (rare<V>(e.type == BF_TRANSMITTER_PHASED)) {
        // phasedtransmitter.cpp:560-585: geom_gain *= W; ds.pdf *= W; ds.pdf = sqrt(ds.pdf^2); extents = 1
        float w = phased_sample_wigner(e.velems, e.n_velems, e.wid, p, -ds.d, lambda0);
        geom_gain *= w;
        ds.pdf *= w;
        ds.pdf = __builtin_sqrtf(ds.pdf * ds.pdf);
        return active ? signal_power * e.gain * geom_gain * 1.f : 0.f;
    }
    float ws = rect_sample_wigner(rc, p, -ds.d, lambda0);
    geom_gain *= ws;
    ds.pdf *= ws;
    float extents = rcp(rc.area) * 6.28318530717958647692f;
    return active ? signal_power * e.gain * geom_gain * extents : 0.f;
}
// Transmitter::pdf_direction — areatransmitter.cpp:167-186, wignertransmitter.cpp:540-577
template <int V = 0> BF_DEV float transmitter_pdf_direction(const DScene &sc, CEmitter &e, V3 p_ref, V3 p_hit, V3 n_hit, float lambda0) {
    CRect &rc = c_rects(sc)[e.rect];
    V3 d = p_hit - p_ref;
    float dist = norm(d);
    d = d / dist;
    float dp = dot(d, n_hit);
    float value = rc.inv_area, adp = __builtin_fabsf(dot(d, n_hit));
    value *= (adp != 0.f) ? (dist * dist) / adp : 0.f;
    if (e.type == BF_TRANSMITTER_WIGNER) value *= rect_sample_wigner(rc, p_hit, -d, lambda0);
    if (rare<V>(e.type == BF_TRANSMITTER_PHASED)) {                // phasedtransmitter.cpp:606-620
        value *= phased_sample_wigner(e.velems, e.n_velems, e.wid, p_hit, -d, lambda0);
        value = __builtin_sqrtf(value * value);
    }
    return (dp < 0.f) ? value : 0.f;
}

// Receiver::sample_ray_differential — omnidirectional.cpp:72-107, wignerreceiver.cpp:208-269
template <int V = 0>
BF_DEV float receiver_sample_ray(const DScene &sc, float time, bool mix, float wl_sample, float px, float py, float ax, float ay, V3 &o, V3 &d,
                                 float &mint, float &maxt, float &lambda0) {
    CSensor &s = c_sensor(sc);
    CRect &rc = c_rects(sc)[s.rect];
    o = xf_point(rc.to_world, mk(px * 2.f - 1.f, py * 2.f - 1.f, 0.f));
    V3 local = square_to_cosine_hemisphere(ax, ay);
    Frame f;
    f.n = mk(rc.n[0], rc.n[1], rc.n[2]);
    coordinate_system(f.n, f.s, f.t);
    d = to_world(f, local);
    mint = kRayEpsilon;
    maxt = BF_INF;
    if ((V & kLean) || s.type == BF_RECEIVER_OMNI) {
        float lo = sc.lambda_min, hi = sc.lambda_max;
        lambda0 = wl_sample * (hi - lo) + lo;            // sample_uniform_spectrum (spectrum.h:312-316), lane 0
        return (hi - lo) * rc.area;
    }
    float freq = wl_sample * s.freq_ext + (s.freq_centre - s.freq_ext / 2);
    float signal_power = 1.f;
    if (mix) {
        // receive_type "mix_resample" (wignerreceiver.cpp:172-189): the receiver's own local oscillator
        if (s.rx_sig_is_delta) {
            // sample_delta_frequency(time) (:149-166): the instantaneous frequency at the sampled receive time, weight 1
            freq = s.freq_centre;
            if (s.rx_signal == BF_SIGNAL_LINFMCW) {
                float t = fmodulo_j(time, rcp_ieee(s.rx_prf));
                float ti = 0 + s.rx_pulse_len / 2;
                freq = s.freq_centre + div_ieee(s.freq_ext, s.rx_pulse_len) * (t - ti);
            }
        } else {
            // the uniform sample above, weighted with eval_signal(time, f) (:118-142)
            signal_power = s.rx_amplitude * s.rx_amplitude;
            if (s.rx_signal != BF_SIGNAL_CW) {
                float t = fmodulo_j(time, rcp_ieee(s.rx_prf));
                float ti = 0 + s.rx_pulse_len / 2;
                float fi = s.rx_signal == BF_SIGNAL_LINFMCW ? s.freq_centre + div_ieee(s.freq_ext, s.rx_pulse_len) * (t - ti) : s.freq_centre;
                signal_power = rect_j((t - ti) / s.rx_pulse_len) > 0.f ? wchirp_j(t - ti, freq - fi, s.rx_pulse_len, s.rx_amplitude) : 0.f;
            }
        }
    }
    lambda0 = (float) ((double) (sc.c * rcp_ieee(freq)) * 1e9);
    if (s.type == BF_RECEIVER_PHASED) {
        // phasedreceiver.cpp:299-365: geom_gain = W(ds) * pdf * (1 - (ds.d . ds.n)^4), ds.d the LOCAL cosine direction
        float w = phased_sample_wigner(s.velems, s.n_velems, s.wid, o, local, lambda0);
        float dn = dot(local, f.n);
        float geom = w * rc.inv_area * (1 - dn * dn * dn * dn);
        float ext = rc.area * kPi;
        if (!s.rx_sig_is_delta) ext = (float) ((double) (ext * (sc.c * rcp(s.freq_ext))) * 1e9);
        return signal_power * s.gain * geom * ext;
    }
    float ws = rect_sample_wigner(rc, o, local, lambda0);   // ds.d is the LOCAL cosine direction (:249-252)
    float geom_gain = ws * rc.inv_area;
    float extents = rc.area * kPi;
    if (!s.rx_sig_is_delta) extents = (float) ((double) (extents * (sc.c * rcp(s.freq_ext))) * 1e9);
    return signal_power * s.gain * geom_gain * extents;
}

BF_NS_END  // namespace bfd
