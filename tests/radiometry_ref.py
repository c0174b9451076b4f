"""Closed-form radiometry for the path estimator: a float64 reference, the scenes it describes and the comparison rule.

Every expectation in this module comes from radiometry (the inverse-square law, configuration factors, the radiosity series of
an enclosure, thermal equilibrium, the directional albedo of a microfacet lobe) and from the reference's DOCUMENTED plugin
weights and conventions, which are cited by file and line (spot.cpp's falloff, irradiancemeter.cpp's and fluxmeter.cpp's ray
weights, path.cpp's depth convention, microfacet.h's distributions).  No number here is the output of any program, and nothing
of the reference is copied: the formulas are restated in numpy, only line numbers are cited.  The module shares no code with
oracle/ or beifong_amd/csrc/; the scene builders use the public scene description (beifong_amd.scenedesc) alone.

The reference half (rect_form_factor, microfacet_albedo, spot_falloff ...) is plain numpy in float64.  The scene builders return
Case(sd, lp, expected, ...); check_statistical / check_deterministic are the rule both test files apply (tests/test_radiometry_host.py on
the oracle, tests/test_gpu_radiometry.py on the device)."""
import functools
import math
from typing import NamedTuple, Optional

import numpy as np

from beifong_amd import capi, scenes
from beifong_amd.scenedesc import SceneDesc, Transform4f
from tests.hist_bound import fp32_sum_bound

T = Transform4f
Z_MAX = 4.5              # two-sided normal tail 6.8e-6 per check; the seeds are fixed, so a run is reproducible
REL_SE_MAX = 0.002       # a 1 % bias is then at least 5 sigma
NONFINITE_MAX = 1e-4     # share of records the film drops (n_invalid)
DET_REL = 1e-5           # deterministic scenes: |L - expected| <= DET_REL * (the closed form without the falloff)


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def _gauss_legendre(lo, hi, order):
    x, w = np.polynomial.legendre.leggauss(order)
    return 0.5 * (hi - lo) * x + 0.5 * (hi + lo), 0.5 * (hi - lo) * w


def _f_corner(a, b, h):
    """Configuration factor from a differential area to a parallel rectangle a x b at height h, one of whose corners lies on
    the element's normal (Howell, A Catalog of Radiation Heat Transfer Configuration Factors, B-4; odd in a and in b)."""
    ra, rb = math.sqrt(a * a + h * h), math.sqrt(b * b + h * h)
    return (a / ra * math.atan(b / ra) + b / rb * math.atan(a / rb)) / (2.0 * math.pi)


def rect_form_factor(px, py, a, b, h):
    """Configuration factor from a differential area at (px, py, 0), normal +z, to the parallel rectangle [-a, a] x [-b, b] at
    height h: the signed four-corner sum of _f_corner (the point may lie outside the rectangle's footprint: the oddness of
    _f_corner does the subtraction)."""
    x0, x1, y0, y1 = -a - px, a - px, -b - py, b - py
    return _f_corner(x1, y1, h) - _f_corner(x0, y1, h) - _f_corner(x1, y0, h) + _f_corner(x0, y0, h)


def rect_form_factor_quadrature(px, py, a, b, h, order=200):
    """The same by brute force: the integral of cos(theta) cos(theta') / (pi r^2) over the rectangle, tensor Gauss-Legendre."""
    x, wx = _gauss_legendre(-a, a, order)
    y, wy = _gauss_legendre(-b, b, order)
    r2 = (x[:, None] - px) ** 2 + (y[None, :] - py) ** 2 + h * h
    return float(np.sum(wx[:, None] * wy[None, :] * h * h / (math.pi * r2 * r2)))


def point_light_radiance(rho, intensity, light, p, n=(0.0, 0.0, 1.0)):
    """Radiance leaving a diffuse surface point p (normal n) lit by an isotropic point light: rho / pi * I cos(theta) / r^2."""
    d = np.asarray(light, np.float64) - np.asarray(p, np.float64)
    r2 = float(d @ d)
    return rho / math.pi * intensity * float(d @ np.asarray(n, np.float64)) / math.sqrt(r2) / r2


def spot_falloff(angle_deg, cutoff_deg, beam_deg):
    """spot.cpp:111-114: 1 inside the beam width, 0 at and beyond the cutoff, in between LINEAR IN THE ANGLE
    (cutoff - angle) / (cutoff - beam width) (:90 the inverse transition width), not in its cosine."""
    if angle_deg <= beam_deg:
        return 1.0
    if angle_deg >= cutoff_deg:
        return 0.0
    return (cutoff_deg - angle_deg) / (cutoff_deg - beam_deg)


def furnace_series(rho, max_depth):
    """Radiance in a closed enclosure whose walls all have reflectance rho and emit 1: sum_{j < max_depth} rho^j.  The depth
    convention is the reference's (path.cpp:124-149): the emitter term is added before the depth test, so max_depth 1 is
    emission alone (exactly 1, no sample drawn) and max_depth d carries d - 1 reflections; -1 is the whole series 1 / (1 - rho)."""
    if max_depth < 0:
        return 1.0 / (1.0 - rho)
    return float(sum(rho ** j for j in range(max_depth)))


def _ndf(mx, my, mz, au, av, distribution):
    """microfacet.h:184-198 (the 1e-20 guard of :201 is below float64's interest)"""
    if distribution == "beckmann":
        c2 = np.maximum(mz * mz, 1e-300)
        e = -((mx / au) ** 2 + (my / av) ** 2) / c2
        # (below e^-200 the lobe is 0 to float64's purposes; clipping keeps exp out of the slow subnormal range)
        return np.where(e > -200.0, np.exp(np.maximum(e, -200.0)) / (math.pi * au * av * c2 * c2), 0.0)
    return 1.0 / (math.pi * au * av * ((mx / au) ** 2 + (my / av) ** 2 + mz * mz) ** 2)


def _smith_g1(vx, vy, vz, mx, my, mz, au, av, distribution):
    """microfacet.h:331-353.  Beckmann: the RATIONAL approximation of :337-342 (1 for a >= 1.6), not the erf form it
    approximates to 0.35 %: the estimator integrates what the reference evaluates.  GGX: :344.  :348 perpendicular incidence
    gives 1, :352 a direction on the other side of the microfacet 0."""
    xy = (au * vx) ** 2 + (av * vy) ** 2
    with np.errstate(divide="ignore", invalid="ignore"):
        t2 = xy / (vz * vz)
        if distribution == "beckmann":
            a = 1.0 / np.sqrt(t2)
            g = np.where(a >= 1.6, 1.0, (3.535 * a + 2.181 * a * a) / (1.0 + 2.276 * a + 2.577 * a * a))
        else:
            g = 2.0 / (1.0 + np.sqrt(1.0 + t2))
    g = np.where(xy == 0.0, 1.0, g)
    return np.where((vx * mx + vy * my + vz * mz) * vz <= 0.0, 0.0, g)


def _albedo_at(theta_i, phi_i, au, av, distribution, n_mu, n_phi, light_pdf=None):
    """light_pdf(ox, oy, oz) (a solid-angle density of the directions wo): the integrand is weighted by the power heuristic's
    weight of visible-normal BSDF sampling against that density, p_b^2 / (p_b^2 + p_l^2) (path.cpp:222-226), p_b = D G1(wi) /
    (4 cos(theta_i)) (roughconductor.cpp:388-389)"""
    wi = np.array([math.sin(theta_i) * math.cos(phi_i), math.sin(theta_i) * math.sin(phi_i), math.cos(theta_i)])
    mu, wm = _gauss_legendre(0.0, 1.0, n_mu)
    # the lobe sits around the mirror direction, azimuth phi_i + pi: centre the azimuthal interval on it
    ph, wp = _gauss_legendre(phi_i, phi_i + 2.0 * math.pi, n_phi)
    cp, sp, total = np.cos(ph)[None, :], np.sin(ph)[None, :], 0.0
    for lo in range(0, n_mu, 128):                       # (rows of cos(theta_o) in slabs: the arrays stay small)
        m, w = mu[lo:lo + 128], wm[lo:lo + 128]
        s = np.sqrt(1.0 - m * m)[:, None]
        ox, oy, oz = s * cp, s * sp, np.broadcast_to(m[:, None], (m.size, n_phi))
        hx, hy, hz = ox + wi[0], oy + wi[1], oz + wi[2]
        inv = 1.0 / np.sqrt(hx * hx + hy * hy + hz * hz)
        hx, hy, hz = hx * inv, hy * inv, hz * inv
        d = _ndf(hx, hy, hz, au, av, distribution)
        g = _smith_g1(wi[0], wi[1], wi[2], hx, hy, hz, au, av, distribution) * _smith_g1(ox, oy, oz, hx, hy, hz, au, av, distribution)
        # roughconductor.cpp:314: the value eval() returns already carries cos(theta_o)
        f = d * g / (4.0 * wi[2])
        if light_pdf is not None:
            pb = d * _smith_g1(wi[0], wi[1], wi[2], hx, hy, hz, au, av, distribution) / (4.0 * wi[2])
            pl = light_pdf(ox, oy, oz)
            with np.errstate(invalid="ignore"):
                f = np.where(pb > 0.0, f * (pb * pb) / (pb * pb + pl * pl), 0.0)
        total += float(np.sum(w[:, None] * wp[None, :] * f))
    return total


def _converged(fn, tol, what):
    n_mu, prev = 100, None
    while n_mu <= 3200:
        cur = fn(n_mu)
        if prev is not None and abs(cur - prev) <= tol:
            return cur
        prev, n_mu = cur, 2 * n_mu
    raise ArithmeticError(f"{what} has not converged to {tol}")


@functools.lru_cache(maxsize=None)
def microfacet_albedo(theta_i, alpha_u, alpha_v, distribution, phi_i=0.0, tol=1e-7):
    """The directional albedo of the rough conductor with Fresnel = 1: the integral of f(wi, wo) cos(theta_o) over the
    hemisphere of wo, wi at polar angle theta_i and azimuth phi_i (radians) of the shading frame (alpha_u along s).

    Restated from the reference's formulas: the normal distributions of microfacet.h:190-198, the Smith G1 of microfacet.h:
    331-353 (for Beckmann the rational approximation of :337-342), G = G1(wi) G1(wo) (:319-321) and roughconductor.cpp:296-314,
    D G / (4 cos(theta_i)) at the half vector normalize(wo + wi).  Tensor Gauss-Legendre in cos(theta_o) and phi; the order is
    doubled until two successive orders agree to tol."""
    return _converged(lambda n: _albedo_at(theta_i, phi_i, alpha_u, alpha_v, distribution, n, 2 * n), tol,
                      f"microfacet_albedo({theta_i}, {alpha_u}, {alpha_v}, {distribution}, {phi_i})")


def beckmann_g1_exact(theta, phi, alpha_u, alpha_v):
    """The Smith G1 of a Beckmann surface in its erf form, 2 / (1 + erf(a) + exp(-a^2) / (a sqrt(pi))), a = 1 / (alpha tan(theta))
    with the roughness projected on the direction as microfacet.h:332-333 does: what the rational form of :337-342 approximates"""
    t2 = ((alpha_u * math.cos(phi)) ** 2 + (alpha_v * math.sin(phi)) ** 2) * math.tan(theta) ** 2
    if t2 == 0.0:
        return 1.0
    a = 1.0 / math.sqrt(t2)
    return 2.0 / (1.0 + math.erf(a) + math.exp(-a * a) / (a * math.sqrt(math.pi)))


def beckmann_visible_ratio(theta, phi, alpha_u, alpha_v):
    """What visible-normal sampling of a Beckmann lobe returns in excess, as a factor: G1_exact(wi) / G1_rational(wi).

    The reference draws the microfacet normal from the EXACT distribution of visible normals (microfacet.h:358-394 inverts the
    erf-form CDF of the visible slopes), whose density is D G1_exact(wi) <wi, m> / cos(theta_i), but states its density (:214-218,
    :311-312) and derives the sample's weight G1(wo) (roughconductor.cpp:234-238) with the rational G1 of :337-342.  The BSDF-
    sampled part of an estimate therefore carries this factor (within 0.35 % of 1, :338; it is 0.9971 at alpha 0.4, 60 deg and
    1.0023 at 80 deg), while emitter sampling, which only evaluates the BSDF, does not.  GGX has its G1 in closed form (:344) and
    samples it exactly: no factor.  This is the reference's behaviour and it is kept: the oracle and the kernels restate both
    halves, and the expectation of a Beckmann lobe under sample_visible carries the factor on its BSDF-sampled share."""
    g = float(_smith_g1(math.sin(theta) * math.cos(phi), math.sin(theta) * math.sin(phi), math.cos(theta), 0.0, 0.0, 1.0,
                        alpha_u, alpha_v, "beckmann"))
    return beckmann_g1_exact(theta, phi, alpha_u, alpha_v) / g


@functools.lru_cache(maxsize=None)
def bsdf_sampled_share(theta_i, alpha_u, alpha_v, distribution, phi_i, light_pdf, tol=1e-5):
    """The part of microfacet_albedo that the power heuristic assigns to visible-normal BSDF sampling when the incident radiance
    is 1 and the lights are sampled with the solid-angle density light_pdf(ox, oy, oz) (_albedo_at)"""
    return _converged(lambda n: _albedo_at(theta_i, phi_i, alpha_u, alpha_v, distribution, n, 2 * n, light_pdf), tol, "bsdf_sampled_share")


# ---------------------------------------------------------------------------------------------------------------------------
# the scenes
# ---------------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    sd: SceneDesc
    lp: capi.bf_launch
    expected: float                   # of the records' mean
    kind: str                         # "deterministic" / "statistical"
    unattenuated: Optional[float] = None     # deterministic: the closed form with the falloff taken as 1 (the yardstick)
    lean: Optional[bool] = None              # whether the device runs the lean kernel build (None: not asserted)
    extra: Optional[dict] = None


def _launch(n_paths, seed_block, max_depth=-1, mode=capi.BF_MODE_PATH, **kw):
    """Seeds of different renders lie n_paths apart (capi.converge_seeds): a seed shifts the path index, so that seeds 1 and 2
    would share all but one path.  seed_block names the block of n_paths streams the render draws from."""
    return capi.make_launch(mode, n_paths, seed=seed_block * n_paths, max_depth=max_depth, rr_depth=5, color_mode=capi.BF_COLOR_MONO, **kw)


def with_paths(lp, n_paths, seed_block=None):
    """A copy of the launch at another path count, its seed moved to the same block of the new size."""
    out = capi.bf_launch.from_buffer_copy(lp)
    block = (lp.seed // lp.n_paths) if seed_block is None else seed_block
    if out.spp:
        pixels = out.film_width * out.film_height
        out.spp = n_paths // pixels
        n_paths = out.spp * pixels
    out.n_paths, out.seed = n_paths, block * n_paths
    return out


def _plate(sd, rho, half=10.0):
    sd.add_rectangle(T.scale([half, half, 1]), sd.add_diffuse(rho))


def point_plate(n_paths=64):
    """A diffuse plate (rho 0.6) at z = 0 under a point light of intensity 40 (point.cpp:80-106: I / r^2), seen by a
    radiance meter: rho / pi * I cos(theta) / r^2, the same float on every path."""
    sd = SceneDesc()
    _plate(sd, 0.6)
    light, p = (0.7, -0.4, 2.0), (0.2, 0.1, 0.0)
    sd.add_point(list(light), intensity=40.0)
    sd.set_radiancemeter(T.look_at([1.0, 1.0, 1.5], list(p), [0, 0, 1]))
    sd.finalize()
    e = point_light_radiance(0.6, 40.0, light, p)
    return Case(sd, _launch(n_paths, 1), e, "deterministic", unattenuated=e)


SPOT_ANGLES = (0.0, 10.0, 17.0, 19.9, 25.0)


def spot_plate(angle_deg, n_paths=64):
    """The same plate under a spot (intensity 40, cutoff 20 deg, beam width 15 deg) at height 2 looking down; the meter aims at
    the plate point seen from the spot at angle_deg off its axis: rho / pi * I * falloff * cos(theta) / r^2 with spot.cpp's
    falloff (spot_falloff), exactly 0 beyond the cutoff."""
    sd = SceneDesc()
    _plate(sd, 0.6)
    sd.add_spot(T.look_at([0, 0, 2.0], [0, 0, 0], [0, 1, 0]), intensity=40.0, cutoff_angle=20.0, beam_width=15.0)
    p = (2.0 * math.tan(math.radians(angle_deg)), 0.0, 0.0)
    sd.set_radiancemeter(T.look_at([p[0] + 0.8, 1.0, 1.5], list(p), [0, 0, 1]))
    sd.finalize()
    u = point_light_radiance(0.6, 40.0, (0.0, 0.0, 2.0), p)
    return Case(sd, _launch(n_paths, 1), u * spot_falloff(angle_deg, 20.0, 15.0), "deterministic", unattenuated=u)


RECT_LIGHTS = (((0.0, 0.0), 0.5, 0.5, 1.0), ((0.8, -0.3), 0.5, 0.25, 0.2), ((2.0, 1.0), 0.3, 0.6, 0.5))
RECT_LIGHT_PATHS = (1 << 14, 1 << 20, 1 << 16)       # the smallest powers of four that meet REL_SE_MAX (the second sees a sliver of the light)


def rect_light(k, max_depth, n_paths=None):
    """A plate (rho 0.7) under a one-sided rectangular light [-a, a] x [-b, b] at height h facing down (radiance 3, rho 0), the
    meter on plate point p: rho * Le * rect_form_factor.  One emitter, MIS of emitter and BSDF sampling; the plate is the only
    reflector, so max_depth 2 and -1 have the same expectation."""
    (px, py), a, b, h = RECT_LIGHTS[k]
    sd = SceneDesc()
    _plate(sd, 0.7)
    light = sd.add_rectangle(T.translate([0, 0, h]) * T.rotate([1, 0, 0], 180) * T.scale([a, b, 1]), sd.add_diffuse(0.0))
    sd.add_area_emitter(light, 3.0)
    # the meter stays below the light's plane, so its ray cannot meet the light
    sd.set_radiancemeter(T.look_at([px + 0.3 * h, py - 0.4 * h, 0.5 * h], [px, py, 0.0], [0, 0, 1]))
    sd.finalize()
    return Case(sd, _launch(n_paths or RECT_LIGHT_PATHS[k], 2 + k, max_depth), 0.7 * 3.0 * rect_form_factor(px, py, a, b, h), "statistical")


# the six inward-facing walls of [-1, 1]^3: -z, +z, -x, +x, -y, +y
_WALLS = (lambda: T.translate([0, 0, -1]), lambda: T.translate([0, 0, 1]) * T.rotate([1, 0, 0], 180),
          lambda: T.translate([-1, 0, 0]) * T.rotate([0, 1, 0], 90), lambda: T.translate([1, 0, 0]) * T.rotate([0, 1, 0], -90),
          lambda: T.translate([0, -1, 0]) * T.rotate([1, 0, 0], -90), lambda: T.translate([0, 1, 0]) * T.rotate([1, 0, 0], 90))
BOX_EYE, BOX_TARGET = (0.3, -0.2, 0.1), (1.0, 0.4, -0.7)


def _box(sd, rhos, radiances):
    for wall, rho, le in zip(_WALLS, rhos, radiances):
        sd.add_area_emitter(sd.add_rectangle(wall(), sd.add_diffuse(rho)), le)


FURNACE_RHOS = (0.5, 0.9)
FURNACE_DEPTHS = (1, 2, 3, 6, 12, -1)


def furnace(rho, max_depth, n_paths=1 << 16):
    """The closed box of six walls, each diffuse rho and an area emitter of radiance 1, a radiance meter inside: furnace_series.
    Six emitters (uniform emitter selection in the light sample AND in the MIS density of a BSDF-sampled hit), a sensor
    inside a closed box, light samples that graze the wall they lie on, Russian roulette beyond depth 5."""
    sd = SceneDesc()
    _box(sd, [rho] * 6, [1.0] * 6)
    sd.set_radiancemeter(T.look_at(list(BOX_EYE), list(BOX_TARGET), [0, 0, 1]))
    sd.finalize()
    return Case(sd, _launch(n_paths, 5, max_depth), furnace_series(rho, max_depth), "deterministic" if max_depth == 1 else "statistical",
                unattenuated=1.0, lean=False)


# the wall with rho 0 lies behind the camera of the film variant (-x), the brightest noise (rho 0.9) in front of it
EQUILIBRIUM_RHOS = (0.2, 0.75, 0.0, 0.9, 0.6, 0.5)
EQUILIBRIUM_L = 2.5
METER_AREA = 0.08
EQUILIBRIUM_SENSORS = ("radiancemeter", "irradiancemeter", "fluxmeter", "film")
EQUILIBRIUM_FILM = (4, 3)


def equilibrium_box(sensor="radiancemeter", n_paths=1 << 16, mode=capi.BF_MODE_PATH, **launch_kw):
    """The same box, wall i with its own reflectance rho_i and radiance 2.5 (1 - rho_i): an enclosure in thermal equilibrium,
    where the radiance is 2.5 at every point in every direction (a wall returns rho_i 2.5 + (1 - rho_i) 2.5), whatever the
    shapes inside, as long as they obey the same rule.

    radiancemeter: 2.5.  film: a perspective camera, 4 x 3 pixels, fov 70 deg: 2.5 in every pixel.  irradiancemeter, fluxmeter:
    a 0.2 x 0.4 rectangle (area 0.08) with rho 0; the ray weights are pi / area (irradiancemeter.cpp:82) and pi
    (fluxmeter.cpp:81-83: both meters draw cosine-distributed directions, whose density cos / pi leaves pi), so the records'
    mean is pi / 0.08 * 2.5 and pi * 2.5.  A sensor's shape is an ordinary surface of the scene: a cold black meter would shadow
    the walls (about 1 % here) and break the equilibrium, so the meter is a black body of the enclosure's temperature: rho 0,
    radiance 2.5 (1 - 0), and since an area emitter emits from its front only it has a twin 1 mm behind it facing the other way."""
    sd = SceneDesc()
    _box(sd, EQUILIBRIUM_RHOS, [EQUILIBRIUM_L * (1.0 - r) for r in EQUILIBRIUM_RHOS])
    film, spp, expected = None, 0, EQUILIBRIUM_L
    if sensor == "radiancemeter":
        sd.set_radiancemeter(T.look_at(list(BOX_EYE), list(BOX_TARGET), [0, 0, 1]))
    elif sensor == "film":
        film = EQUILIBRIUM_FILM
        sd.set_perspective(T.look_at(list(BOX_EYE), list(BOX_TARGET), [0, 0, 1]), fov=70.0, near_clip=0.01, far_clip=100.0, film=film)
        spp = n_paths // (film[0] * film[1])
        n_paths = spp * film[0] * film[1]
    else:
        pose = T.translate([-0.3, 0.2, -0.2]) * T.rotate([0.3, 1.0, 0.2], 35.0)
        meter = sd.add_rectangle(pose * T.scale([0.1, 0.2, 1]), sd.add_diffuse(0.0))
        sd.add_area_emitter(meter, EQUILIBRIUM_L)
        back = sd.add_rectangle(pose * T.translate([0, 0, -1e-3]) * T.rotate([1, 0, 0], 180) * T.scale([0.1, 0.2, 1]), sd.add_diffuse(0.0))
        sd.add_area_emitter(back, EQUILIBRIUM_L)
        if sensor == "irradiancemeter":
            sd.set_irradiancemeter(meter)
            expected = math.pi / METER_AREA * EQUILIBRIUM_L
        else:
            sd.set_fluxmeter(meter)
            expected = math.pi * EQUILIBRIUM_L
    sd.finalize()
    return Case(sd, _launch(n_paths, 7, -1, mode=mode, film=film, spp=spp, **launch_kw), expected, "statistical", lean=False)


def equilibrium_film_range(rfilter, n_paths):
    """equilibrium_box's 4 x 3 film through the range integrator (16 bins of 1 m), under the box filter or the default Gaussian
    reconstruction filter (gaussian.cpp: stddev 0.5, radius 2 pixels), discretised by the oracle as bf_sensor.rfilter carries it"""
    from tests.scene_builders import oracle_rfilter
    case = equilibrium_box("film", n_paths, mode=capi.BF_MODE_RANGE, bins=16, bin_width=1.0)
    if rfilter == "gaussian":
        case.sd.sensor.rfilter = oracle_rfilter("gaussian", 0.5)
        case.sd.finalize()
    return case


ALBEDO_CASES = tuple((d, (a, a), t, sv) for d in ("beckmann", "ggx") for a in (0.1, 0.4) for t in (0.0, 60.0, 80.0) for sv in (True, False)) + \
    (("ggx", (0.05, 0.4), 60.0, True),)
ALBEDO_AZIMUTH = 30.0       # of the meter in the patch's frame: the anisotropic lobe is seen off its axes


def albedo(distribution, alphas, theta_deg, sample_visible, n_paths=1 << 16):
    """The uniform furnace (rho 0.5, radiance 1) with a 0.6 x 0.6 rough-conductor patch (Fresnel 1: eta 0, k 1) at z = -0.5, a
    radiance meter 0.4 from its centre at polar angle theta, azimuth 30 deg, max_depth 2: the patch reflects the walls' emission
    once, radiance 1 from every direction of its hemisphere, so the meter reads microfacet_albedo.  A narrow lobe against six
    large lights: the MIS weights decide here.  One idiosyncrasy of the reference is part of the expectation: Beckmann under
    sample_visible (beckmann_visible_ratio)."""
    sd = SceneDesc()
    _box(sd, [0.5] * 6, [1.0] * 6)
    sd.add_rectangle(T.translate([0, 0, -0.5]) * T.scale([0.3, 0.3, 1]),
                     sd.add_roughconductor(alpha=alphas[0], alpha_v=alphas[1], distribution=distribution, sample_visible=sample_visible))
    th, ph = math.radians(theta_deg), math.radians(ALBEDO_AZIMUTH)
    eye = [0.4 * math.sin(th) * math.cos(ph), 0.4 * math.sin(th) * math.sin(ph), -0.5 + 0.4 * math.cos(th)]
    sd.set_radiancemeter(T.look_at(eye, [0, 0, -0.5], [0, 1, 0]))
    sd.finalize()
    expected = microfacet_albedo(th, alphas[0], alphas[1], distribution, ph)
    if distribution == "beckmann" and sample_visible:
        # the reference's visible-normal sampling of a Beckmann lobe (beckmann_visible_ratio), on the BSDF-sampled share
        expected += (beckmann_visible_ratio(th, ph, *alphas) - 1.0) * bsdf_sampled_share(th, alphas[0], alphas[1], distribution, ph, _furnace_light_pdf)
    return Case(sd, _launch(n_paths, 11, 2), expected, "statistical", lean=False)


def _furnace_light_pdf(ox, oy, oz):
    """The solid-angle density with which the furnace's six walls are sampled from the albedo patch's centre (0, 0, -0.5), for
    directions of the upper hemisphere: a uniformly chosen wall (1 / 6, scene.cpp:180-230), a uniform point on it (1 / 4), and
    dist^2 / cos at the wall (shape.cpp:332-337).  The direction meets exactly one wall of [-1, 1]^3."""
    with np.errstate(divide="ignore"):
        tx, ty, tz = 1.0 / np.abs(ox), 1.0 / np.abs(oy), 1.5 / np.abs(oz)
    t = np.minimum(np.minimum(tx, ty), tz)
    cos_wall = np.where(t == tx, np.abs(ox), np.where(t == ty, np.abs(oy), np.abs(oz)))
    return t * t / (24.0 * cos_wall)


FRONTEND_CASES = ((0.5, 0.3), (2.0, 0.8), (5.0, 0.8))         # (range r, plate reflectance)
FRONTEND_PLATES = ("rectangle", "mesh", "mesh_normals")
FRONTEND_BINS, FRONTEND_DR = 256, 0.1
FRONTEND_APERTURE = (20e-3, 50e-3)                            # half-widths of scenes._radar_frontend's 40 x 100 mm aperture
FRONTEND_FOV = 45.0
FRONTEND_RADIANCE = 1000.0


def _grid_mesh(corner, eu, ev, n=9):
    """An n x n-vertex grid over the parallelogram corner + s eu + t ev, two triangles per cell"""
    s = np.linspace(0.0, 1.0, n)
    v = np.array([np.asarray(corner) + a * np.asarray(eu) + b * np.asarray(ev) for b in s for a in s], np.float32)
    f = []
    for j in range(n - 1):
        for i in range(n - 1):
            k = j * n + i
            f += [[k, k + 1, k + n + 1], [k, k + n + 1, k + n]]
    return v, np.array(f, np.uint32)


def frontend_plate_expected(r, rho, order=96):
    """The pixel mean of rho * Le * rect_form_factor(hit) over the film: the perspective camera spreads the film uniformly over
    the square [-tan(fov / 2), tan(fov / 2)]^2 of the plane at distance 1, so over a square of half-width r tan(fov / 2) of the
    plate, which faces the aperture at distance r."""
    t = r * math.tan(math.radians(FRONTEND_FOV / 2))
    x, w = _gauss_legendre(-t, t, order)
    a, b = FRONTEND_APERTURE
    ff = np.array([[rect_form_factor(xi, yj, a, b, r) for yj in x] for xi in x])
    return rho * FRONTEND_RADIANCE * float(np.sum(w[:, None] * w[None, :] * ff)) / (4.0 * t * t)


def frontend_longest_path(r):
    """The largest value the range integrator's path length can take in frontend_plate.  A path that returns light has two
    segments: sensor to plate (t1) and plate to aperture (t2).  t1 <= r sqrt(1 + 2 tan^2(fov / 2)) (a corner of the film); t2 <=
    the distance from that corner of the lit square to the far corner of the aperture.  pathlength.cpp adds every
    segment once when it is traced (:146, :307), the first again at the emitter sample (:209) and the second again when the
    path stands on the emitter (:161), so the recorded length is 2 t1 for a path lit by its emitter sample and at most 2 (t1 + t2); the lower end, 2 t1 >= 2 r,
    is what puts the return in the bin of the two-way range."""
    t = r * math.tan(math.radians(FRONTEND_FOV / 2))
    a, b = FRONTEND_APERTURE
    t1 = math.sqrt(r * r + 2.0 * t * t)
    t2 = math.sqrt(r * r + (t + a) ** 2 + (t + b) ** 2)
    return 2.0 * (t1 + t2)


def frontend_plate(r, rho, plate="rectangle", n_paths=1 << 18):
    """scenes._radar_frontend (the C2 monostatic front end: an aperture light of radiance 1000 looking along +x, a perspective
    receiver with fov 45 deg at the same place) and a diffuse plate of half-width 4 r at range r, in BF_MODE_RANGE, 256 bins of
    0.1 m, max_depth 2.  The plate as a rectangle, as a 9 x 9-vertex mesh, and as that mesh with (flat) vertex normals: the
    same expectation; the mesh forms go through the BVH."""
    sd = SceneDesc()
    scenes._radar_frontend(sd, radiance=FRONTEND_RADIANCE)
    x, z0, hw = r, 0.3, 4.0 * r
    mat = sd.add_diffuse(rho)
    if plate == "rectangle":
        sd.add_rectangle(T.translate([x, 0, z0]) * T.rotate([0, 1, 0], -90) * T.scale([hw, hw, 1]), mat)      # normal -x
    else:
        # counter-clockwise seen from the sensor (geometric normal -x)
        v, f = _grid_mesh([x, -hw, z0 - hw], [0, 0, 2 * hw], [0, 2 * hw, 0])
        normals = np.tile(np.array([-1.0, 0.0, 0.0], np.float32), (len(v), 1)) if plate == "mesh_normals" else None
        sd.add_mesh(v, f, mat, normals=normals)
    sd.finalize()
    lp = _launch(n_paths, 13, 2, mode=capi.BF_MODE_RANGE, bins=FRONTEND_BINS, bin_width=FRONTEND_DR)
    return Case(sd, lp, frontend_plate_expected(r, rho), "statistical", lean=True, extra=dict(r=r))


# ---------------------------------------------------------------------------------------------------------------------------
# the comparison rule
# ---------------------------------------------------------------------------------------------------------------------------
class Estimate(NamedTuple):
    mean: float
    se: float
    z: float
    n: int
    nonfinite: int


def estimate(L, expected):
    """mean, standard error and z of the finite records, in float64"""
    L = np.asarray(L, np.float64)
    x = L[np.isfinite(L)]
    mean = float(x.mean())
    se = float(x.std(ddof=1) / math.sqrt(x.size))
    z = (mean - expected) / se if se > 0.0 else (0.0 if mean == expected else math.copysign(math.inf, mean - expected))
    return Estimate(mean, se, z, x.size, L.size - x.size)


def check_statistical(L, expected, what, log=None):
    """The three conditions of a statistical scene, on the per-path records: |mean - expected| <= 4.5 se; se <= 0.2 % of the
    expectation (a condition on the test: n_paths is chosen to meet it); at most 1e-4 of the records not finite."""
    e = estimate(L, expected)
    line = f"{what}: mean {e.mean:.7g} expected {expected:.7g} se {e.se:.3g} (rel {e.se / abs(expected):.2e}) z {e.z:+.2f} non-finite {e.nonfinite} of {e.n + e.nonfinite}"
    if log is not None:
        log(line)
    assert e.nonfinite <= NONFINITE_MAX * (e.n + e.nonfinite), line
    assert e.se <= REL_SE_MAX * abs(expected), line
    assert abs(e.mean - expected) <= Z_MAX * e.se, line
    return e


def check_deterministic(L, case, what, log=None):
    """Every record the same float, within 1e-5 of the unattenuated closed form of the expectation (exactly 0 where the closed form is 0)"""
    L = np.asarray(L)
    assert L.size and np.all(L.view(np.uint32) == L.view(np.uint32)[0]), f"{what}: the paths differ"
    err = abs(float(L[0]) - case.expected)
    line = f"{what}: L {float(L[0]):.9g} expected {case.expected:.9g} |diff| {err:.3g} = {err / case.unattenuated:.3g} U"
    if log is not None:
        log(line)
    if case.expected == 0.0:
        assert float(L[0]) == 0.0, line
    assert err <= DET_REL * case.unattenuated, line
    return err / case.unattenuated


# The one sampler stream of these tests whose first float, the film position's x offset, is exactly 0: path 612323 of seed block 7
# at 2^20 paths (path p of a launch draws from stream seed + path_offset + p).  Under the box filter ImageBlock::put places it one
# pixel to the left of its own (dropped_finite): on a 1 x 1 film, or in column 0, that is outside the film and the sample is
# dropped although it is finite.  Every equilibrium_box launch at 2^20 paths contains it.
ZERO_X_STREAMS = (7 * (1 << 20) + 612323,)


def zero_x_paths(lp):
    """the paths of the launch that draw a film position with x exactly 0 (ZERO_X_STREAMS)"""
    first = int(lp.seed) + int(lp.path_offset)
    return [s - first for s in ZERO_X_STREAMS if 0 <= s - first < int(lp.n_paths)]


def allowed_dropped(lp):
    """how many finite samples the box-filtered film of this launch drops: its zero_x_paths that lie in column 0"""
    if not lp.spp:
        return len(zero_x_paths(lp))
    return sum(1 for p in zero_x_paths(lp) if (p // lp.spp) % lp.film_width == 0)


def dropped_finite(n_invalid, L, allowed=0):
    """How many samples the film dropped although their record is finite, and the most they can have carried.  n_invalid counts
    what ImageBlock::put refuses: the non-finite samples, and under the box filter a sample whose film position is exactly 0 in x or
    y (imageblock.cpp:113,166-172: lo = ceil(pos - 0.5 - 0.5) = -1 is outside the block; the position is the path's first two
    sampler floats, each 0 with probability 2^-24 or so).  That number must be `allowed` (allowed_dropped: 0 in every launch that does not
    contain the stream named in ZERO_X_STREAMS), so that a film which loses a finite sample is noticed.  The records do not say which finite sample went, so
    a sum over them is bounded with the d largest magnitudes."""
    L = np.asarray(L, np.float64)
    fin = np.abs(L[np.isfinite(L)])
    d = int(n_invalid) - (L.size - fin.size)
    assert d == allowed and n_invalid <= NONFINITE_MAX * L.size, (n_invalid, L.size - fin.size, allowed)
    top = np.sort(fin)[fin.size - d:] if d else np.zeros(0)
    return d, float(top.sum()), float((top * top).sum())


def check_film_mean(hist, L, n_invalid, what, allowed=0, x=0, w=4):
    """hist[X] / hist[W] of a BF_COLOR_MONO render against the records: W counts the samples the film kept (exactly), X is an
    fp32 sum of their records, so it lies within the fp32 summation bound (tests/hist_bound.py) of the float64 sum of the finite
    records, less what the film dropped of them (dropped_finite)."""
    L = np.asarray(L, np.float64)
    fin = L[np.isfinite(L)]
    h = np.asarray(hist, np.float64)
    d, top, _ = dropped_finite(n_invalid, L, allowed)
    assert h[w] == L.size - n_invalid, (what, h[w], L.size, n_invalid)
    bound = float(fp32_sum_bound(np.abs(fin).sum(), np.count_nonzero(fin)))
    assert -bound - top <= h[x] - fin.sum() <= bound, (what, h[x], fin.sum(), bound, d, top)
    return h[x] / h[w]


def check_film_pixels(hist, L, case, what, value_channel=0, box=True, log=None):
    """A multi-pixel film: every pixel's value / W within 4.5 of its own se of the expectation, nothing added to that allowance.
    The se comes from the pixel's own records (path g belongs to pixel g // spp).

    box=True (the box filter: a pixel's samples are its own paths, each with weight 1) ties the film to the records in a separate
    assertion, as check_film_mean does for the 1 x 1 film: the pixel's W is the number of its finite records, exactly, and its
    value channel an fp32 sum of them, within the summation bound sized by the pixel's own addends.  (The film puts a path of
    zero_x_paths one pixel to the left, or drops it in column 0; the tie follows it there.)"""
    lp = case.lp
    px = lp.film_width * lp.film_height
    L = np.asarray(L, np.float64).reshape(px, lp.spp)
    h = np.asarray(hist, np.float64).reshape(px, -1)
    worst = 0.0
    lands = np.repeat(np.arange(px), lp.spp)               # the pixel whose cells a path's sample is added to
    for g in zero_x_paths(lp):
        lands[g] = lands[g] - 1 if lands[g] % lp.film_width else -1
    flat = L.reshape(-1)
    for p in range(px):
        fin = L[p][np.isfinite(L[p])]
        se = float(fin.std(ddof=1) / math.sqrt(fin.size))
        value = h[p, value_channel] / h[p, 4]
        line = f"{what} pixel {p}: {value:.7g} se {se:.3g} z {(value - case.expected) / se if se else 0.0:+.2f}"
        if log is not None:
            log(line)
        assert se > 0.0 and abs(value - case.expected) <= Z_MAX * se, line
        if box:
            fin = flat[(lands == p) & np.isfinite(flat)]
            assert h[p, 4] == fin.size, (line, h[p, 4], fin.size)
            bound = float(fp32_sum_bound(np.abs(fin).sum(), np.count_nonzero(fin)))
            assert abs(h[p, value_channel] - fin.sum()) <= bound, (line, h[p, value_channel], fin.sum(), bound)
        worst = max(worst, abs(value - case.expected) / se)
    return worst


def check_range_profile(hist, rec, case, what):
    """The exact facts of frontend_plate's range profile.  The bins sum to the radiance channel: both are fp32 sums of the same
    addends (the perspective sensor's ray weight is 1 and the launch is BF_COLOR_MONO), so they differ by at most twice the
    summation bound.  Every bin below floor(2 r / dr) is exactly 0: no return is nearer than the two-way range.  Every bin
    beyond the longest path the geometry allows (frontend_longest_path, plus 1e-5 of it for the fp32 distances) is exactly 0."""
    r, lp = case.extra["r"], case.lp
    h = np.asarray(hist, np.float64)
    bins = h[5:]
    L = np.asarray(rec["L"], np.float64)
    assert np.all(np.isfinite(L))
    bound = float(fp32_sum_bound(np.abs(L).sum(), np.count_nonzero(L)))
    assert bins.size == lp.bins and abs(bins.sum() - h[0]) <= 2.0 * bound, (what, bins.sum(), h[0], bound)
    first = int(math.floor(2.0 * r / FRONTEND_DR + 1e-9))
    assert not bins[:first].any(), (what, np.flatnonzero(bins[:first]))
    longest = frontend_longest_path(r) * (1.0 + 1e-5)
    last = int(math.floor(longest / FRONTEND_DR))
    assert last + 1 < lp.bins and not bins[last + 1:].any(), (what, last, np.flatnonzero(bins[last + 1:]))
    assert bins[first] > 0.0, what                       # the plate's centre returns in the bin of 2 r
    aux = np.asarray(rec["aux"], np.float64)[L != 0.0]
    assert aux.min() >= 2.0 * r and aux.max() <= longest, (what, aux.min(), aux.max())
