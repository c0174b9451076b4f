"""The CPU oracle's path estimator against closed-form radiometry (tests/radiometry_ref.py).

Every other test of the estimator compares the kernels with the oracle, and the oracle with the reference in pieces; the value
a render returns is checked here against numbers that come from radiometry alone.  The rule (radiometry_ref.check_*):
deterministic scenes to 1e-5 of the unattenuated closed form, every path the same float; statistical scenes |mean - expected|
<= 4.5 se from the per-path records, with se <= 0.2 % of the expectation and at most 1e-4 of the records not finite.  The path
counts are the smallest powers of two at which every case of a group meets the se condition, except in the closed boxes: the
cap on non-finite records can only be judged where one record lies below it, so they run at 2^16 or more (_furnace_paths).

What the scenes separate: emission alone (furnace, max_depth 1); one bounce under a delta light (point_plate, spot_plate); MIS
with one emitter (rect_light); MIS with six emitters and the emitter-selection probability (furnace, equilibrium_box, albedo);
the geometric series in depth and the depth convention (furnace); Russian roulette, beyond depth 5 only (furnace 6 against 12
and -1, equilibrium_box); the sensors' ray weights (equilibrium_box); the range integrator's film (frontend_plate)."""
import math

import numpy as np
import pytest

from beifong_amd import capi
from tests import radiometry_ref as rr
from tests.oracle_lib import OracleScene

THREADS = 16


def _render(case, **kw):
    return OracleScene(case.sd).render(case.lp, records=True, threads=THREADS, **kw)


def _statistical(case, what):
    hist, rec, st = _render(case)
    e = rr.check_statistical(rec["L"], case.expected, what, print)
    rr.dropped_finite(st.n_invalid, rec["L"], rr.allowed_dropped(case.lp))
    if not case.lp.spp:
        rr.check_film_mean(hist, rec["L"], st.n_invalid, what, rr.allowed_dropped(case.lp))
    return hist, rec, st, e


# ---- the reference module's own checks ----
@pytest.mark.parametrize("k", range(3))
def test_form_factor_against_quadrature(k):
    """the corner-sum closed form against the double integral of cos cos' / (pi r^2); configurations 1 and 2 have the point
    outside the rectangle's footprint (two, respectively all four corner terms change sign)"""
    (px, py), a, b, h = rr.RECT_LIGHTS[k]
    assert (abs(px) > a or abs(py) > b) == (k > 0)
    f, q = rr.rect_form_factor(px, py, a, b, h), rr.rect_form_factor_quadrature(px, py, a, b, h)
    assert 0.0 < f < 1.0 and abs(f - q) <= 1e-12, (f, q)
    # the unoccluded limit: a point far below a small rectangle sees A cos^2 / (pi r^2)
    far = rr.rect_form_factor(0.0, 0.0, 1e-3, 2e-3, 10.0)
    assert abs(far / (8e-6 / (math.pi * 100.0)) - 1.0) < 1e-7


@pytest.mark.parametrize("distribution", ["beckmann", "ggx"])
def test_albedo_tends_to_one(distribution):
    """normal incidence: G1(wi) = 1 and the lobe narrows onto the mirror direction, so the albedo rises to 1 as alpha falls"""
    a = [rr.microfacet_albedo(0.0, al, al, distribution) for al in (0.4, 0.2, 0.1, 0.05)]
    assert all(x <= y + 1e-9 and y <= 1.0 + 1e-9 for x, y in zip(a, a[1:])) and a[0] < a[2], a
    assert 1.0 - a[-1] < (1e-6 if distribution == "beckmann" else 5e-3), a


@pytest.mark.parametrize("distribution", ["beckmann", "ggx"])
def test_albedo_symmetry(distribution):
    """swapping (alpha_u, alpha_v) and turning the azimuth by 90 degrees is a rotation of the surface about its normal"""
    th, ph = math.radians(60.0), math.radians(30.0)
    a = rr.microfacet_albedo(th, 0.05, 0.4, distribution, ph)
    b = rr.microfacet_albedo(th, 0.4, 0.05, distribution, ph + math.pi / 2)
    assert abs(a - b) <= 2e-7, (a, b)
    assert abs(a - rr.microfacet_albedo(th, 0.05, 0.4, distribution, math.pi / 2)) > 1e-3        # (the lobe IS anisotropic)


def test_beckmann_g1_forms():
    """the erf form of the Beckmann G1 against the rational form the reference evaluates: within the 0.35 % microfacet.h:338
    states, equal to 1e-3 only where both are near 1, and the ratio the albedo scenes carry"""
    worst = 0.0
    for deg in range(1, 90):
        for alpha in (0.05, 0.1, 0.4, 1.0):
            r = rr.beckmann_visible_ratio(math.radians(deg), 0.3, alpha, alpha)
            worst = max(worst, abs(r - 1.0))
    assert 2e-3 < worst < 3.5e-3, worst
    assert rr.beckmann_visible_ratio(0.0, 0.0, 0.4, 0.4) == 1.0
    assert abs(rr.beckmann_visible_ratio(math.radians(60.0), 0.5, 0.4, 0.4) - 0.99710) < 1e-5
    assert abs(rr.beckmann_visible_ratio(math.radians(80.0), 0.5, 0.4, 0.4) - 1.00232) < 1e-5


# ---- deterministic scenes ----
@pytest.mark.parametrize("angle", [None] + list(rr.SPOT_ANGLES))
def test_delta_lights(angle):
    """One bounce under a delta light: every path the same float, within 1e-5 U of rho / pi I falloff cos / r^2, U the closed
    form without the falloff (an fp32 acos error is divided by the 5 degree transition width).

    Measured on the oracle, |L - expected| / U: point_plate 2.2e-7; spot 0 deg 9.1e-9, 10 deg 9.2e-8, 17 deg 1.2e-6, 19.9 deg 1.9e-6
    (the worst case; the bound is five times that), 25 deg exactly 0."""
    case = rr.point_plate() if angle is None else rr.spot_plate(angle)
    hist, rec, st = _render(case)
    rr.check_deterministic(rec["L"], case, f"delta light {angle}", print)
    assert st.n_invalid == 0 and hist[4] == case.lp.n_paths
    if angle == 25.0:
        assert case.expected == 0.0 and not rec["L"].any()
    if angle in (17.0, 19.9):
        # linear in the angle, not in its cosine: the cosine form would read 0.6116 and 0.0209 of the full beam here
        assert abs(case.expected / case.unattenuated - (20.0 - angle) / 5.0) < 1e-12


def test_furnace_depth_one_is_emission_alone():
    """path.cpp:124-149: max_depth 1 returns the emitter term of the first hit and draws nothing: exactly 1 on every path"""
    for rho in rr.FURNACE_RHOS:
        case = rr.furnace(rho, 1, n_paths=256)
        hist, rec, st = _render(case)
        assert case.expected == 1.0 and np.all(rec["L"] == np.float32(1.0)) and st.n_rays_shadow == 0 and st.n_bounces == 0


# ---- statistical scenes ----
@pytest.mark.parametrize("max_depth", [2, -1])
@pytest.mark.parametrize("k", range(3))
def test_rect_light(k, max_depth):
    _statistical(rr.rect_light(k, max_depth), f"rect_light[{k}, {max_depth}]")


def _furnace_paths(rho, max_depth):
    """2^13 would meet the se condition in most cases, but the cap on non-finite records can only be judged where one record is
    below it (n > 1e4; the boxes lose about one path in 3e4 to 1e5): the closed boxes run at 2^16 or more"""
    return 1 << (18 if (rho, max_depth) == (0.9, -1) else 16)


@pytest.mark.parametrize("max_depth", [d for d in rr.FURNACE_DEPTHS if d != 1])
@pytest.mark.parametrize("rho", rr.FURNACE_RHOS)
def test_furnace(rho, max_depth):
    _statistical(rr.furnace(rho, max_depth, _furnace_paths(rho, max_depth)), f"furnace[{rho}, {max_depth}]")


@pytest.mark.parametrize("sensor", rr.EQUILIBRIUM_SENSORS)
def test_equilibrium_box(sensor):
    case = rr.equilibrium_box(sensor, 1 << 16)
    hist, rec, st, e = _statistical(case, f"equilibrium_box[{sensor}]")
    if sensor == "film":
        rr.check_film_pixels(hist, rec["L"], case, "equilibrium film (oracle)")


@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
def test_equilibrium_film_in_range_mode(rfilter):
    """the film through the range integrator and a wide reconstruction filter: every pixel's Y / W within 4.5 of its own se of 2.5"""
    case = rr.equilibrium_film_range(rfilter, 1 << 18)
    hist, rec, st, e = _statistical(case, f"equilibrium film {rfilter}")
    rr.check_film_pixels(hist, rec["L"], case, f"equilibrium film {rfilter} (oracle)", value_channel=1, box=rfilter == "box", log=print)


@pytest.mark.parametrize("case_id", range(len(rr.ALBEDO_CASES)))
def test_albedo(case_id):
    dist, alphas, theta, sv = rr.ALBEDO_CASES[case_id]
    _statistical(rr.albedo(dist, alphas, theta, sv, 1 << (17 if sv else 18)), f"albedo[{dist}, {alphas}, {theta}, visible={sv}]")


@pytest.mark.parametrize("theta", [60.0, 80.0])
def test_beckmann_visible_normal_sampling_is_the_reference_s(theta):
    """A finding of these tests, kept as the reference's behaviour (radiometry_ref.beckmann_visible_ratio).  Beckmann, alpha 0.4,
    sample_visible, at 2^20 paths: the estimator does NOT return the albedo of the BSDF it evaluates; it is off by -0.26 % at
    60 deg and +0.22 % at 80 deg (z = -7.3 and +7.6 here), because the reference samples the exact distribution of visible normals
    (microfacet.h:358-394) and weights the sample with the rational G1 (microfacet.h:337-342, roughconductor.cpp:234-238).  With
    the factor G1_exact / G1_rational on the BSDF-sampled share the expectation is met (z = -0.1 and +0.1); without
    sample_visible nothing of the kind is seen (test_albedo).  An estimator "corrected" to the plain albedo would differ from
    the reference."""
    case = rr.albedo("beckmann", (0.4, 0.4), theta, True, 1 << 20)
    hist, rec, st, e = _statistical(case, f"beckmann visible {theta}")
    th, ph = math.radians(theta), math.radians(rr.ALBEDO_AZIMUTH)
    plain = rr.estimate(rec["L"], rr.microfacet_albedo(th, 0.4, 0.4, "beckmann", ph))
    print(f"against the plain albedo: z {plain.z:+.2f}")
    assert abs(plain.z) > rr.Z_MAX and (plain.z > 0) == (rr.beckmann_visible_ratio(th, ph, 0.4, 0.4) > 1.0)


@pytest.mark.parametrize("plate", rr.FRONTEND_PLATES)
@pytest.mark.parametrize("r,rho", rr.FRONTEND_CASES)
def test_frontend_plate(r, rho, plate):
    """Measured on the oracle: z = +0.29, +0.47, +0.49 for the three ranges at these 2^13 paths (+0.40, +0.33, +0.31 at 2^16); the
    three plate forms trace the same paths, record for record."""
    case = rr.frontend_plate(r, rho, plate, 1 << 13)
    hist, rec, st, e = _statistical(case, f"frontend_plate[{r}, {rho}, {plate}]")
    rr.check_range_profile(hist, rec, case, f"frontend_plate[{r}, {plate}]")


def test_frontend_expectation_by_two_quadratures():
    for r, rho in rr.FRONTEND_CASES:
        assert abs(rr.frontend_plate_expected(r, rho, 96) / rr.frontend_plate_expected(r, rho, 48) - 1.0) < 1e-12


def test_second_seed_block():
    """the rule on disjoint sample sets: seeds n_paths apart (capi.converge_seeds) share no path"""
    case = rr.equilibrium_box("radiancemeter", 1 << 16)
    seeds = capi.converge_seeds(case.lp, 3)
    assert int(seeds[1] - seeds[0]) == case.lp.n_paths
    means = []
    for block in (20, 21):
        c = case._replace(lp=rr.with_paths(case.lp, 1 << 16, block))
        means.append(_statistical(c, f"equilibrium_box seed block {block}")[3].mean)
    assert means[0] != means[1]


def test_nonfinite_records_are_the_power_heuristic_of_a_grazing_light_sample():
    """The closed boxes return a few non-finite records (2 to 14 per 2^18 to 2^20 paths, a share of at most 1.4e-5; the film drops
    them and n_invalid counts them).  Two of them replayed alone (path_offset, n_paths 1): the same NaN; finite up to some
    max_depth d - 1 and NaN from d >= 2 on, so the NaN is born in an emitter-sampling step, never in the emission term.

    Read against the reference: a light sample drawn on the wall the path stands on has dot(d, n) of a few 1e-20 or less
    (the walls' rotations carry cos(90 deg) = 6e-17 in fp32), shape.cpp:336-337 divides dist^2 by it, ds.pdf passes 1.8e19 or is
    inf, path.cpp:222-226 squares it to inf and returns inf / (inf + pdf_b^2) = NaN (pdf_a > 0 selects the quotient), and
    path.cpp:171 adds mis * throughput * bsdf_val * emitter_val = NaN * ... * 0.  The reference evaluates the same fp32
    expressions, so it returns NaN there too and ImageBlock::put drops the sample: behaviour kept, not a defect."""
    case = rr.furnace(0.9, -1, 1 << 18)
    o = OracleScene(case.sd)
    hist, rec, st = o.render(case.lp, records=True, threads=THREADS)
    bad = np.flatnonzero(~np.isfinite(rec["L"]))
    assert 2 <= bad.size <= rr.NONFINITE_MAX * case.lp.n_paths and st.n_invalid == bad.size
    for i in bad[:2]:
        one = capi.bf_launch.from_buffer_copy(case.lp)
        one.n_paths, one.path_offset = 1, int(i)
        h1, r1, s1 = o.render(one, records=True)
        assert np.isnan(r1["L"][0]) and np.isnan(rec["L"][i]) and s1.n_invalid == 1 and h1[4] == 0.0
        born = None
        for depth in range(1, 64):
            one.max_depth = depth
            if np.isnan(o.render(one, records=True)[1]["L"][0]):
                born = depth
                break
        print(f"path {i}: NaN from max_depth {born}")
        assert born is not None and born >= 2


def test_zero_x_stream_draws_a_film_position_of_zero(oracle):
    """radiometry_ref.ZERO_X_STREAMS: the first sampler float of that stream, the film position's x offset, is exactly 0, and the
    box-filtered 1 x 1 film drops the (finite) sample: the one case in which n_invalid exceeds the non-finite records"""
    import ctypes as C
    out = np.ones(2, np.float32)
    oracle.bfo_sampler_floats(C.c_uint64(rr.ZERO_X_STREAMS[0]), 2, out.ctypes.data_as(C.c_void_p))
    assert out[0] == 0.0 and out[1] > 0.0
    case = rr.equilibrium_box("radiancemeter", 1 << 20)
    (p,) = rr.zero_x_paths(case.lp)
    one = capi.bf_launch.from_buffer_copy(case.lp)
    one.n_paths, one.path_offset = 1, p
    assert rr.allowed_dropped(case.lp) == 1 and rr.allowed_dropped(one) == 1 and rr.allowed_dropped(rr.with_paths(case.lp, 1 << 16)) == 0
    hist, rec, st = OracleScene(case.sd).render(one, records=True)
    assert np.isfinite(rec["L"][0]) and rec["L"][0] > 0 and st.n_invalid == 1 and hist[4] == 0.0
