"""Expected values of a BF_FLAG_CLASSES render, built from what the oracle exports without knowing about classes.

The class of a path is shape_class[s], s the shape of its first intersection, or miss_class if its first ray leaves the scene.
first_hits composes that intersection from three oracle exports, in the order generate_path draws its samples:

    bfo_sampler_floats(seed + path_offset + p, 4) -> fx, fy, ax, ay   (ax, ay only if the sensor is neither perspective nor
                                                                       radiance meter: they are .5 otherwise)
    OracleScene.sensor_sample_ray(x, y, ax, ay)   -> o, mint, d       (x, y: fx, fy on the 1 x 1 film; ((q % W) + fx) / W,
                                                                       ((q // W) + fy) / H in float32 for pixel q =
                                                                       (path_offset + p) // spp of a W x H film without crop)
    OracleScene.trace_closest([o, mint, d, inf])  -> t, shape

The oracle's sensor_sample_ray has no receiver branch; a receiver's ray geometry is the flux meter's, so receive scenes are
composed on a TWIN description (fluxmeter_twin) and traced on either.  Two self-checks pin the composition: its hit / miss
equals record.valid of the oracle's render of the launch for every path, and every composed t of a perspective sensor lies
below far_clip (the composed ray has none).

per_class then renders every path alone on the oracle (as moment_ref.single_paths does) and accumulates ref, S, N per class; its
bookkeeping is held to the oracle's Addends of the whole launch.  check holds every class block of a device histogram to
hist_bound.assert_fp32_sum.
"""
import ctypes as C

import numpy as np

from beifong_amd import capi
from tests import oracle_lib
from tests.hist_bound import assert_fp32_sum, assert_two_fp32_sums, count_channels
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene


def classed(lp, extra=0):
    return copy_launch(lp, flags=lp.flags | capi.BF_FLAG_CLASSES | extra)


def film_scene():
    """scenes.bus_radar(n_tris=2000) seen through an 8 x 6 film"""
    from beifong_amd import scenes
    from beifong_amd.scenedesc import Transform4f as T
    sd, _ = scenes.bus_radar(n_tris=2000)
    d0 = T.rotate([0, 0, 1], 0.0) * T.rotate([1, 0, 0], 90) * T.rotate([0, 1, 0], 90)
    sd.set_perspective(T.translate([0.0, 0.0, 0.3]) * d0, fov=45.0, near_clip=0.1, far_clip=100.0, film=(8, 6))
    sd.finalize()
    lp = capi.make_launch(capi.BF_MODE_RANGE, 8 * 6 * 64, seed=7, bins=64, bin_width=0.4, color_mode=capi.BF_COLOR_RGB, film=(8, 6), spp=64)
    return sd, lp


def receive_scene(n_paths=4096):
    """scenes.bus_receive on a 2000-triangle bus, 64 time bins"""
    from beifong_amd import scenes
    return scenes.bus_receive(n_tris=2000, n_paths=n_paths, t_bins=64, dr=0.4, seed=5)


def fluxmeter_twin(build):
    """`build()` once more, its receiver replaced by a flux meter on the same rectangle: what first_hits composes receive-mode
    rays on.  Returns the twin description."""
    sd = build()
    sd = sd[0] if isinstance(sd, tuple) else sd
    sd.set_fluxmeter(int(sd.sensor.shape))
    sd.finalize()
    return sd


def first_hits(sd, lp, twin=None, records=None, trace_sd=None):
    """(shape, hit) of every path of launch `lp` on description `sd`: int64 shape index of the first intersection (-1: none)
    and whether there is one.  `twin`: the description the sensor rays are composed on (receive scenes); `records`: the
    oracle's records of the launch if the caller has them (else rendered here); `trace_sd`: the description the rays are
    traced on (default `sd`: a posed copy has the same sensor)."""
    lib = oracle_lib.load()
    n = int(lp.n_paths)
    compose = OracleScene(twin if twin is not None else sd)
    sensor = (twin if twin is not None else sd).sensor
    pinhole = sensor.type in (capi.BF_SENSOR_PERSPECTIVE, capi.BF_SENSOR_RADIANCEMETER)
    film = bool(lp.spp and lp.film_width and lp.film_height)
    if film:
        assert sensor.crop_offset_x == 0 and sensor.crop_offset_y == 0, "first_hits composes films without a crop"
    W, H = (np.float32(lp.film_width), np.float32(lp.film_height)) if film else (np.float32(1), np.float32(1))
    rays = np.zeros((n, 8), np.float32)
    u = np.zeros(4, np.float32)
    for p in range(n):
        lib.bfo_sampler_floats(C.c_uint64(lp.seed + lp.path_offset + p), 4, u.ctypes.data_as(C.c_void_p))
        fx, fy = np.float32(u[0]), np.float32(u[1])
        ax, ay = (0.5, 0.5) if pinhole else (float(u[2]), float(u[3]))
        x, y = fx, fy
        if film:
            q = (lp.path_offset + p) // lp.spp
            x = (np.float32(q % lp.film_width) + fx) / W
            y = (np.float32(q // lp.film_width) + fy) / H
        r = compose.sensor_sample_ray(float(x), float(y), ax, ay)
        rays[p, 0:3], rays[p, 3], rays[p, 4:7], rays[p, 7] = r["o"], r["mint"], r["d"], np.inf
    t, _, shape, _ = OracleScene(trace_sd if trace_sd is not None else sd).trace_closest(rays)
    hit = np.isfinite(t)
    if records is None:
        records = OracleScene(trace_sd if trace_sd is not None else sd).render(lp, records=True, threads=8)[1]
    valid = records["valid"] != 0
    assert np.array_equal(hit, valid), f"composed first hit differs from record.valid for {int((hit != valid).sum())} of {n} paths"
    if sensor.type == capi.BF_SENSOR_PERSPECTIVE and hit.any():
        assert float(t[hit].max()) < float(sensor.far_clip), (float(t[hit].max()), float(sensor.far_clip))
    return np.where(hit, shape.astype(np.int64), -1), hit


def path_classes(shape, shape_class, miss_class):
    """class of every path from first_hits' shape indices"""
    sc = np.asarray(shape_class, np.int64)
    return np.where(shape >= 0, sc[np.maximum(shape, 0)], int(miss_class))


class Expected(object):
    """ref, S, N of every class block ([n_classes, channels]) of one classed render, and the plain launch's count channels"""

    def __init__(self, ref, S, N, counts, cls):
        self.ref, self.S, self.N, self.counts, self.cls = ref, S, N, counts, cls
        self.n_classes = ref.shape[0]

    def population(self):
        return np.bincount(self.cls, minlength=self.n_classes)

    def merged(self, groups):
        """the expectation of a table that maps class k of this one to class groups[k]"""
        g = np.asarray(groups, np.int64)
        m = int(g.max()) + 1
        ref, S, N = (np.zeros((m,) + a.shape[1:], a.dtype) for a in (self.ref, self.S, self.N))
        for k in range(self.n_classes):
            ref[g[k]] += self.ref[k]
            S[g[k]] += self.S[k]
            N[g[k]] += self.N[k]
        return Expected(ref, S, N, self.counts, g[self.cls])

    def check(self, hist, what):
        """every class block of a device histogram against its expected cells: N = 0 cells (every cell of an unpopulated class
        among them) exactly 0, count channels exact per class"""
        h = np.asarray(hist).reshape(self.n_classes, -1)
        assert h.shape == self.ref.shape, (what, h.shape, self.ref.shape)
        return max(assert_fp32_sum(h[k], self.ref[k], self.S[k], self.N[k], f"{what}, class {k}", counts=self.counts)
                   for k in range(self.n_classes))

    def check_two(self, h1, h2, what):
        a, b = (np.asarray(h).reshape(self.n_classes, -1) for h in (h1, h2))
        return max(assert_two_fp32_sums(a[k], b[k], self.S[k], self.N[k], f"{what}, class {k}", counts=self.counts)
                   for k in range(self.n_classes))


def single_path_hists(sd, lp):
    """every path of launch `lp` rendered alone by the oracle (n_paths = 1, path_offset = p): a list of (cells, addends) with
    the non-zero cells of path p's histogram.  A launch of fewer paths, same seed and offset, is a prefix of the list."""
    osc = OracleScene(sd)
    one = copy_launch(lp, n_paths=1, flags=lp.flags & ~capi.BF_FLAG_CLASSES)
    out = []
    for p in range(int(lp.n_paths)):
        one.path_offset = lp.path_offset + p
        h = osc.render(one)[0].astype(np.float64)
        nz = np.flatnonzero(h)
        out.append((nz, h[nz]))
    return out


def per_class(sd, lp, cls, n_classes, addends=None, singles=None):
    """Expected class blocks of launch `lp` (no class flag) on description `sd`, `cls` the class of every path: each path
    rendered alone by the oracle (`singles`: single_path_hists of this launch or of a longer one, if the caller has them),
    accumulated into its class.  The sums over the classes are held to the oracle's Addends of the whole launch (`addends`,
    rendered here if None): N exactly, ref and S to the rounding of 2 n float64 additions."""
    lp = copy_launch(lp, flags=lp.flags & ~capi.BF_FLAG_CLASSES)
    if addends is None:
        addends = OracleScene(sd).render(lp, threads=8, addends=True)[3]
    if singles is None:
        singles = single_path_hists(sd, lp)
    n, n_paths = addends.ref.size, int(lp.n_paths)
    ref, S, N = np.zeros((n_classes, n)), np.zeros((n_classes, n)), np.zeros((n_classes, n), np.int64)
    for p in range(n_paths):
        nz, x = singles[p]
        k = int(cls[p])
        ref[k, nz] += x
        S[k, nz] += np.abs(x)
        N[k, nz] += 1
    assert np.array_equal(N.sum(0), addends.N.astype(np.int64)), "per-class N does not add up to the launch's"
    tol = 2.0 * (n_paths + n_classes) * 2.0 ** -53 * addends.S
    assert np.all(np.abs(ref.sum(0) - addends.ref) <= tol), "per-class ref does not add up to the launch's"
    assert np.all(np.abs(S.sum(0) - addends.S) <= tol), "per-class S does not add up to the launch's"
    return Expected(ref, S, N, count_channels(lp, sd), np.asarray(cls[:n_paths], np.int64))


def expected(sd, lp, shape_class, n_classes, miss_class, twin=None, singles=None):
    """first_hits + per_class of one launch: (Expected, oracle records, Addends of the plain launch)"""
    plain = copy_launch(lp, flags=lp.flags & ~capi.BF_FLAG_CLASSES)
    _, rec, _, add = OracleScene(sd).render(plain, records=True, threads=8, addends=True)
    shape, _ = first_hits(sd, plain, twin=twin, records=rec)
    cls = path_classes(shape, shape_class, miss_class)
    return per_class(sd, plain, cls, n_classes, addends=add, singles=singles), rec, add
