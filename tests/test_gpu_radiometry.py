"""The device's path estimator against closed-form radiometry (tests/radiometry_ref.py), through every kernel route.

Per scene: (1) per-path parity with the oracle at 2^16 paths (new shapes for the parity suite: a sensor inside a closed box, six
area emitters, light samples that graze the wall they lie on, NaN records that both sides must drop alike); (2) the closed form
from the device's own records at 2^20 paths, by the rule of tests/test_radiometry_host.py: |mean - expected| <= 4.5 se, se <=
0.2 % of the expectation, at most 1e-4 of the records not finite, and hist[X] / hist[W] tied to the records by the fp32
summation bound.  frontend_plate runs the lean kernel build, the six-emitter boxes the general one, so both are held to a
closed form."""
import math

import numpy as np
import pytest

from beifong_amd import capi
from tests import radiometry_ref as rr
from tests.hist_bound import FTZ_SLACK, assert_fp32_sum, count_channels, fp32_sum_bound, gamma
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import same_records_by_kind

pytestmark = pytest.mark.gpu
N_PARITY = 1 << 16
N_FORM = 1 << 20


def _parity(g, case, what, n_paths=N_PARITY):
    lp = rr.with_paths(case.lp, n_paths)
    ho, ro, so, add = OracleScene(case.sd).render(lp, records=True, threads=16, addends=True)
    hg, rg, sg = g.render(lp, records=True)
    same_records_by_kind(rg, ro, what)
    assert sg.n_rays_closest == so.n_rays_closest and sg.n_rays_shadow == so.n_rays_shadow, what
    assert sg.n_bounces == so.n_bounces and sg.n_invalid == so.n_invalid, what
    assert_fp32_sum(hg, add.ref, add.S, add.N, what, counts=count_channels(lp, case.sd))
    return sg


def _variant(case, st, what):
    if case.lean is not None:
        assert bool(st.kernel_variant & capi.BF_VARIANT_LEAN) == case.lean, (what, st.kernel_variant)


def _closed_form(g, case, what, n_paths=N_FORM, flags=0):
    lp = rr.with_paths(case.lp, n_paths)
    lp.flags |= flags
    hist, rec, st = g.render(lp, records=True)
    if case.kind == "deterministic":
        rr.check_deterministic(rec["L"], case, what, print)
        assert st.n_invalid == 0
    else:
        rr.check_statistical(rec["L"], case.expected, what, print)
        rr.dropped_finite(st.n_invalid, rec["L"], rr.allowed_dropped(lp))
    if not lp.spp and not flags & capi.BF_FLAG_MOMENT:
        rr.check_film_mean(hist, rec["L"], st.n_invalid, what, rr.allowed_dropped(lp))
    return hist, rec, st, lp


def _both(case, what):
    g = capi.Scene(case.sd)
    _variant(case, _parity(g, case, what + " (parity)"), what)
    out = _closed_form(g, case, what + " (device)", n_paths=case.lp.n_paths if case.kind == "deterministic" else N_FORM)
    _variant(case, out[2], what)
    g.close()
    return out


@pytest.mark.parametrize("angle", [None] + list(rr.SPOT_ANGLES))
def test_delta_lights(hiplib, angle):
    """every path the same float, within 1e-5 U (tests/test_radiometry_host.py::test_delta_lights has the oracle's figures; the
    device's records are bit-equal to them)"""
    case = rr.point_plate() if angle is None else rr.spot_plate(angle)
    g = capi.Scene(case.sd)
    _parity(g, case, f"delta light {angle}", n_paths=case.lp.n_paths)
    _closed_form(g, case, f"delta light {angle}", n_paths=1 << 12)
    g.close()


@pytest.mark.parametrize("max_depth", [2, -1])
@pytest.mark.parametrize("k", range(3))
def test_rect_light(hiplib, k, max_depth):
    _both(rr.rect_light(k, max_depth), f"rect_light[{k}, {max_depth}]")


@pytest.mark.parametrize("max_depth", rr.FURNACE_DEPTHS)
@pytest.mark.parametrize("rho", rr.FURNACE_RHOS)
def test_furnace(hiplib, rho, max_depth):
    hist, rec, st, lp = _both(rr.furnace(rho, max_depth), f"furnace[{rho}, {max_depth}]")
    if max_depth == 1:
        assert np.all(rec["L"] == np.float32(1.0)) and st.n_rays_shadow == 0


@pytest.mark.parametrize("sensor", rr.EQUILIBRIUM_SENSORS)
def test_equilibrium_box(hiplib, sensor):
    case = rr.equilibrium_box(sensor)
    hist, rec, st, lp = _both(case, f"equilibrium_box[{sensor}]")
    if sensor == "film":
        rr.check_film_pixels(hist, rec["L"], case._replace(lp=lp), "equilibrium film", log=print)


@pytest.mark.parametrize("case_id", range(len(rr.ALBEDO_CASES)))
def test_albedo(hiplib, case_id):
    dist, alphas, theta, sv = rr.ALBEDO_CASES[case_id]
    _both(rr.albedo(dist, alphas, theta, sv), f"albedo[{dist}, {alphas}, {theta}, visible={sv}]")


@pytest.mark.parametrize("plate", rr.FRONTEND_PLATES)
@pytest.mark.parametrize("r,rho", rr.FRONTEND_CASES)
def test_frontend_plate(hiplib, r, rho, plate):
    case = rr.frontend_plate(r, rho, plate)
    hist, rec, st, lp = _both(case, f"frontend_plate[{r}, {rho}, {plate}]")
    assert st.kernel_variant & capi.BF_VARIANT_LEAN
    rr.check_range_profile(hist, rec, case, f"frontend_plate[{r}, {plate}]")


# ---- the routes of one launch ----
ROUTES = ["default", "no_tail", "small_pool", "megakernel", "global_atomics"]
ROUTE_SCENES = {"furnace": lambda: rr.furnace(0.9, -1), "equilibrium_box": lambda: rr.equilibrium_box("radiancemeter"),
                "albedo": lambda: rr.albedo("ggx", (0.1, 0.1), 60.0, True)}


@pytest.mark.parametrize("scene", list(ROUTE_SCENES))
def test_routes(hiplib, monkeypatch, scene):
    """The routes of tests/test_gpu_classes.py::test_routes_of_one_launch: the tail kernel, wf_shade / wf_trace to the end, a pool
    of 1024 slots that regenerate, the one-kernel variant, global atomics.  rho 0.9 gives a mean path length of 10 with a long
    Russian-roulette tail, so the tail and the regeneration carry real weight.  Every route against the closed form, and the
    routes pairwise by their records."""
    case = ROUTE_SCENES[scene]()
    n = 1 << (18 if scene == "furnace" else 17)           # (four times what the se condition needs; the small pool makes 2^20 slow)
    records = {}
    for route in ROUTES:
        with monkeypatch.context() as m:
            if route == "no_tail":
                m.setenv("BF_WF_TAIL", "0")
            if route == "small_pool":
                m.setenv("BF_WF_POOL", "1024")
            g = capi.Scene(case.sd)            # (after setenv: the tunables are read when the scene is created)
        flags = {"megakernel": capi.BF_FLAG_MEGAKERNEL, "global_atomics": capi.BF_FLAG_GLOBAL_ATOMICS}.get(route, 0)
        hist, rec, st, lp = _closed_form(g, case, f"{scene} route {route}", n_paths=n, flags=flags)
        assert not st.kernel_variant & capi.BF_VARIANT_LEAN and st.n_paths == n, route
        if route == "no_tail":
            assert st.n_bounces_tail == 0
        if scene != "albedo":                  # (albedo's paths end after one bounce, max_depth 2: nothing is left for a tail)
            if route == "no_tail":
                assert st.n_bounce_iters > 1
            if route == "default":
                assert st.n_bounces_tail > 0
        for other, ro in records.items():
            same_records_by_kind(rec, ro, f"{scene}: route {route} against {other}")
        records[route] = rec
        g.close()
    assert len(records) == len(ROUTES)


# ---- the flags that change arithmetic or accumulation ----
FLAG_SCENES = {"equilibrium_box": lambda: rr.equilibrium_box("radiancemeter"), "frontend_plate": lambda: rr.frontend_plate(2.0, 0.8, "mesh")}


@pytest.mark.parametrize("scene", list(FLAG_SCENES))
def test_fast_arithmetic(hiplib, scene):
    """BF_FLAG_FAST: other roundings, the same estimator: the same rule from its own records"""
    case = FLAG_SCENES[scene]()
    g = capi.Scene(case.sd)
    hist, rec, st, lp = _closed_form(g, case, f"{scene} fast", flags=capi.BF_FLAG_FAST)
    assert st.kernel_variant & capi.BF_VARIANT_FAST
    g.close()


@pytest.mark.parametrize("scene", list(FLAG_SCENES))
def test_exact_sum(hiplib, scene):
    """BF_FLAG_EXACT_SUM: hist[X] is the exact sum of the finite records rounded once to fp32, hist[W] their number, so
    hist[X] / hist[W] is the float64 mean of the records up to that one rounding"""
    case = FLAG_SCENES[scene]()
    g = capi.Scene(case.sd)
    hist, rec, st, lp = _closed_form(g, case, f"{scene} exact sum", flags=capi.BF_FLAG_EXACT_SUM)
    g.close()
    assert st.kernel_variant & capi.BF_VARIANT_EXACT_SUM
    L = rec["L"].astype(np.float64)
    fin = L[np.isfinite(L)]
    total = math.fsum(fin)
    d = rr.dropped_finite(st.n_invalid, rec["L"], rr.allowed_dropped(lp))[0]
    assert hist[4] == lp.n_paths - st.n_invalid
    if d == 0:
        assert hist[0] == np.float32(total), (hist[0], total)
        assert abs(float(hist[0]) / float(hist[4]) - total / fin.size) <= 2.0 ** -24 * abs(total / fin.size)
    else:
        # the film dropped one finite sample (its film position is exactly 0, radiometry_ref.dropped_finite): the cell is the
        # exact sum without one of the records, rounded once
        assert d == 1 and np.any(np.float32(total - fin) == hist[0]), (d, hist[0], total)


@pytest.mark.parametrize("scene", list(FLAG_SCENES))
def test_moment(hiplib, scene):
    """BF_FLAG_MOMENT: capi.moment_estimate's mean +- 4.5 of its own standard error contains the closed form, and that standard
    error is the records'.  With n = n_paths (moment_estimate's n on a 1 x 1 film), m1 = sum L and m2 = sum L^2 over the finite
    records, v = m2 / n - (m1 / n)^2 and se^2 = v / (n - 1).  The device's m1 is an fp32 sum of N addends, within b1 =
    gamma_{N-1} S1 of it (tests/hist_bound.py); its m2 an fp32 sum of the N rounded squares, within b2 = gamma_N S2 (tests/
    moment_ref.py).  So |v_dev - v| <= b2 / n + (2 |m1| b1 + b1^2) / n^2 = dv, and |se_dev^2 - se^2| <= dv / (n - 1).  (Where no
    record is dropped, se is std(L, ddof=1) / sqrt(n), the number check_statistical works with.)"""
    case = FLAG_SCENES[scene]()
    g = capi.Scene(case.sd)
    hist, rec, st, lp = _closed_form(g, case, f"{scene} moment", flags=capi.BF_FLAG_MOMENT)
    g.close()
    assert st.kernel_variant & capi.BF_VARIANT_MOMENT
    mean, var, rel = capi.moment_estimate(hist, lp)
    pair = (lp.bins if lp.mode == capi.BF_MODE_RANGE else 0) + 1            # nested.Y (BF_COLOR_MONO: the radiance itself)
    mean, se = float(mean[0, pair]), math.sqrt(float(var[0, pair]))
    print(f"{scene} moment: mean {mean:.7g} se {se:.3g} z {(mean - case.expected) / se:+.2f}")
    assert abs(mean - case.expected) <= rr.Z_MAX * se and se <= rr.REL_SE_MAX * case.expected
    L = rec["L"].astype(np.float64)
    L = L[np.isfinite(L)]
    n, N = float(lp.n_paths), int(np.count_nonzero(L))
    m1, m2 = float(L.sum()), float((L * L).sum())
    d, top1, top2 = rr.dropped_finite(st.n_invalid, rec["L"], rr.allowed_dropped(lp))          # (finite samples the film dropped: at most the d largest)
    b1 = float(fp32_sum_bound(np.abs(L).sum(), N)) + top1
    b2 = float(gamma(N) * m2 + 2.0 * N * FTZ_SLACK) + top2
    dv = b2 / n + (2.0 * abs(m1) * b1 + b1 * b1) / (n * n)
    se2 = (m2 / n - (m1 / n) ** 2) / (n - 1.0)
    assert abs(se * se - se2) <= dv / (n - 1.0), (se * se, se2, dv / (n - 1.0))


def test_converge(hiplib):
    """render_converge to a relative standard error of 0.01: the mean lands within 4.5 * 0.01 * 2.5 of 2.5 before max_rounds"""
    case = rr.equilibrium_box("radiancemeter", n_paths=64)
    g = capi.Scene(case.sd)
    max_rounds = 64
    hist, rounds, history, n_sig, st = g.render_converge(case.lp, 0.01, max_rounds=max_rounds)
    g.close()
    first, second, w = capi.converge_layout(case.lp)
    mean = float(hist[first[0, 0]]) / float(hist[w[0, 0]])
    print(f"converge: rounds {rounds} history {history} mean {mean:.6g} paths {hist[w[0, 0]]}")
    assert 2 <= rounds < max_rounds and n_sig == 1
    assert abs(mean - rr.EQUILIBRIUM_L) <= rr.Z_MAX * 0.01 * rr.EQUILIBRIUM_L


@pytest.mark.parametrize("rfilter", ["box", "gaussian"])
def test_equilibrium_film_in_range_mode(hiplib, rfilter):
    """The 4 x 3 film through the range integrator, with the box filter and with the default Gaussian (stddev 0.5, radius 2):
    every pixel's Y / W within 4.5 of its own se of 2.5, and parity with the oracle"""
    case = rr.equilibrium_film_range(rfilter, N_FORM)
    g = capi.Scene(case.sd)
    _parity(g, case, f"equilibrium film {rfilter} (parity)")
    hist, rec, st = g.render(case.lp, records=True)
    rr.check_statistical(rec["L"], case.expected, f"equilibrium film {rfilter}", print)
    rr.check_film_pixels(hist, rec["L"], case, f"equilibrium film {rfilter}", value_channel=1, box=rfilter == "box", log=print)
    g.close()
