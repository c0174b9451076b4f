"""Expected values of a BF_FLAG_CLASSES render under a range-rate table (Scene.set_range_rate_classes), from the unchanged oracle.

The class of a path is capi.range_rate_classes(d, p, shape, bins, twists): d the direction of its primary ray, shape and p the shape
and the world-space point of its first intersection.  first_points() composes the primary ray exactly as arrival_ref.directions does
(sampler floats -> sensor_sample_ray; receive scenes on their flux-meter twin), takes shape from OracleScene.trace_closest and p from
OracleScene.intersect_full on the description the launch renders, and keeps the self-check: the composed ray's hit / miss equals
record.valid of the oracle's render for every path.  expected() then hands the classes to class_ref.per_class, which renders every
path alone on the oracle.
"""
import ctypes as C

import numpy as np

from beifong_amd import capi, motion
from tests import class_ref, oracle_lib
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene


def first_points(sd, lp, twin=None, records=None, trace_sd=None):
    """(d float32[n, 3], p float32[n, 3], shape int64[n]) of every path of launch `lp` on description `sd`: the direction of its
    primary ray, the point and the shape index of its first intersection (shape -1, p zeros: none).  `twin`: the description the
    sensor rays are composed on (receive scenes: class_ref.fluxmeter_twin); `records`: the oracle's records of the launch if the
    caller has them (else rendered here); `trace_sd`: the description the rays are traced on (default `sd`: a posed copy has the
    same sensor)."""
    lib = oracle_lib.load()
    n = int(lp.n_paths)
    compose = OracleScene(twin if twin is not None else sd)
    sensor = (twin if twin is not None else sd).sensor
    pinhole = sensor.type in (capi.BF_SENSOR_PERSPECTIVE, capi.BF_SENSOR_RADIANCEMETER)
    film = bool(lp.spp and lp.film_width and lp.film_height)
    if film:
        assert sensor.crop_offset_x == 0 and sensor.crop_offset_y == 0, "first_points composes films without a crop"
    W, H = (np.float32(lp.film_width), np.float32(lp.film_height)) if film else (np.float32(1), np.float32(1))
    rays = np.zeros((n, 8), np.float32)
    u = np.zeros(4, np.float32)
    for i in range(n):
        lib.bfo_sampler_floats(C.c_uint64(lp.seed + lp.path_offset + i), 4, u.ctypes.data_as(C.c_void_p))
        fx, fy = np.float32(u[0]), np.float32(u[1])
        ax, ay = (0.5, 0.5) if pinhole else (float(u[2]), float(u[3]))
        x, y = fx, fy
        if film:
            q = (lp.path_offset + i) // lp.spp
            x = (np.float32(q % lp.film_width) + fx) / W
            y = (np.float32(q // lp.film_width) + fy) / H
        r = compose.sensor_sample_ray(float(x), float(y), ax, ay)
        rays[i, 0:3], rays[i, 3], rays[i, 4:7], rays[i, 7] = r["o"], r["mint"], r["d"], np.inf
    tracer = OracleScene(trace_sd if trace_sd is not None else sd)
    t, _, shape, _ = tracer.trace_closest(rays)
    hit = np.isfinite(t)
    if records is None:
        plain = copy_launch(lp, flags=lp.flags & ~capi.BF_FLAG_CLASSES)
        records = tracer.render(plain, records=True, threads=8)[1]
    valid = records["valid"] != 0
    assert np.array_equal(hit, valid), f"composed first hit differs from record.valid for {int((hit != valid).sum())} of {n} paths"
    p = np.zeros((n, 3), np.float32)
    for i in np.flatnonzero(hit):
        si = tracer.intersect_full(rays[i])
        assert si["t"] == t[i], (i, si["t"], t[i])
        p[i] = si["p"]
    return rays[:, 4:7].copy(), p, np.where(hit, shape.astype(np.int64), -1)


def still(sd):
    """every shape of `sd` at rest"""
    return np.stack([motion.twist() for _ in range(len(sd.shapes))])


# What the tests install (tests/test_range_rate_host.py asserts the populations, tests/test_gpu_range_rate.py renders them).  The radar
# drives along +x at 4 m/s, the apertures ride with it in name only (no path meets them first), the ground is still, and the bus, the
# last shape of every scene, closes at 2 m/s, drifts sideways and yaws at 0.8 rad/s about (10, 3, 1.7): the ground's rates fill [-4, 0),
# the bus's about [-9, -3.4].
SENSOR_LIN = (4.0, 0.0, 0.0)
BUS_TWIST = dict(lin=(-2.0, -0.5, 0.0), ang=(0.0, 0.0, 0.8), pivot=(10.0, 3.0, 1.7))
TABLES = {
    "narrow": ((-6.0, -2.0), 8),          # rates outside on both sides
    "wide": ((-8.0, 0.0), 16),            # a power-of-two window: sr = 2 exactly
    "half": ((-8.0, 0.0), 8),             # "wide" with its bins merged in pairs: sr = 1
    "film": ((-6.0, -3.0), 6),
    "global": ((-7.0, -3.5), 7),
}
# the populations of the tables on the scenes of the GPU tests, as DESIGN.md 6h records them: (bins, outside, miss)
POPULATIONS = {
    ("receive", "narrow"): ([37, 23, 14, 15, 476, 426, 320, 275], 777, 1733),
    ("receive", "wide"): ([62, 44, 61, 36, 37, 23, 14, 15, 476, 426, 320, 275, 219, 150, 108, 28], 69, 1733),
    ("receive", "half"): ([106, 97, 60, 29, 902, 595, 369, 136], 69, 1733),
    ("film", "film"): ([113, 157, 122, 119, 1531, 8], 166, 856),
    ("global", "global"): ([12, 189, 198, 163, 117, 88, 2048], 24, 1257),
}


def table(name, sensor_lin=SENSOR_LIN):
    window, n = TABLES[name]
    return capi.range_rate_bins(window, n, sensor_lin=sensor_lin)


def twists(sd):
    """every shape at rest but the last one, the bus"""
    tw = still(sd)
    tw[len(sd.shapes) - 1] = motion.twist(**BUS_TWIST)
    return tw


def two_plates():
    """scenes.plate_doppler (wavelength 0.1 m, 2^16 paths, with the ground) and a second plate of the same size one metre beside the
    first, at the same range: the scene of the two-target motion sweeps.  Returns (sd, lp, [the two plates' shape indices])."""
    from beifong_amd import scenes
    sd, lp = scenes.plate_doppler(wavelength_m=0.1, n_paths=1 << 16, ground=True)
    k0 = [k for k, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH][0]
    s = sd.shapes[k0]
    p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()
    f = np.ctypeslib.as_array(s.indices, shape=(s.n_faces, 3)).copy()
    p[:, 1] += 1.0
    sd.add_mesh(p, f, sd.add_diffuse(0.8, twosided=True))
    sd.finalize()
    return sd, lp, [k0, len(sd.shapes) - 1]


def expected(sd, lp, bins, twists, twin=None, singles=None, trace_sd=None):
    """first_points + range_rate_classes + class_ref.per_class of one launch: (Expected, oracle records, Addends of the plain
    launch).  `trace_sd`: the posed description the launch renders (the rays are composed on `sd` / `twin`, whose sensor is the
    same; p is the posed point)."""
    plain = copy_launch(lp, flags=lp.flags & ~capi.BF_FLAG_CLASSES)
    on = trace_sd if trace_sd is not None else sd
    _, rec, _, add = OracleScene(on).render(plain, records=True, threads=8, addends=True)
    d, p, shape = first_points(sd, plain, twin=twin, records=rec, trace_sd=trace_sd)
    cls = capi.range_rate_classes(d, p, shape, bins, twists)
    return class_ref.per_class(on, plain, cls, capi.range_rate_n_classes(bins), addends=add, singles=singles), rec, add
