"""Expected values of a BF_FLAG_CLASSES render under a range-rate table whose meshes carry per-vertex velocities
(Scene.set_velocity_mode), from the unchanged oracle.

The class of a path is capi.range_rate_classes(d, p, shape, bins, twists, vertex_velocity=U, has_velocity=has): d, p and shape as
tests/range_rate_ref.py composes them, U = capi.interpolate_velocity(uv, V0, V1, V2) at the barycentrics OracleScene.trace_closest
reports for the path's primary ray, V0..V2 the velocities of the corners of the face it hit.  The face within the shape is the
oracle's primitive index minus the primitives of the shapes before it (a rectangle counts one, a mesh its faces).  first_hits()
keeps range_rate_ref.first_points' self-check: the composed ray's hit / miss equals record.valid of the oracle's render for every
path.  expected() hands the classes to class_ref.per_class, which renders every path alone on the oracle.

The scene of the tests is tests/test_gpu_skin.py's _range_scene(False), restated here: the radar front end, the ground, a
976-triangle bus and the 304-triangle three-bone bar, 8192 paths of seed 3.
"""
import collections
import ctypes as C
import functools

import numpy as np

from beifong_amd import capi, meshgen, motion, scenes
from beifong_amd.scenedesc import SceneDesc
from tests import class_ref, oracle_lib
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene

f32 = np.float32
N_PATHS = 1 << 13
DT = 1.0 / 64.0
WINDOW, N_BINS = (-1.0, 0.0), 8
# the bar's first hits on the scene posed by bend(S, POSES[0]) with the field differenced to bend(S, POSES[1]) over DT, all twists
# zero and the radar at rest, as DESIGN.md 6h records them: (bins, outside).  Of the 250 outside, 8 close faster than 1 m/s and 242
# have a rate of 0 or more: 166 of those lie on the triangles of the root bone alone, which stand still, and a rate of exactly 0 is
# the window's open upper edge.
POSES = ([20.0, -30.0], [21.0, -32.0])
BAR_POPULATION = ([83, 56, 41, 47, 65, 60, 40, 65], 250)
BAR_PRIM0, BAR_HITS = 978, 707

Skin = collections.namedtuple("Skin", "k rest rest_n faces index weight joints n_bones")


def _verts(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()


def faces(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.indices, shape=(s.n_faces, 3)).astype(np.int64)


def range_scene(n_paths=N_PATHS):
    """(sd, lp, S): the scene, its range-mode launch and the bar's skin"""
    sd = SceneDesc()
    scenes._radar_frontend(sd)
    scenes._ground(sd)
    mat = sd.add_roughconductor(alpha=0.1, twosided=True, specular_reflectance=1.0)
    v, f = meshgen.bus(600, seed=1)
    sd.add_mesh(meshgen.place(v, -20.0, (12.0, 3.0, 1.7)), f, mat)
    n_bones = 3
    bv, bf, index, weight = meshgen.jointed_bar(n_bones, 8, 6, radius=0.4)
    joints = np.stack([np.arange(n_bones + 1, dtype=np.float64), np.zeros(n_bones + 1), np.zeros(n_bones + 1)], -1)
    sd.add_mesh(meshgen.place(bv, 75.0, (6.0, -1.5, 0.9)), bf, mat)
    k = len(sd.shapes) - 1
    sd.finalize()
    lp = capi.make_launch(capi.BF_MODE_RANGE, n_paths, seed=3, bins=1024, bin_width=0.03)
    S = Skin(k, _verts(sd, k), None, bf, index, weight, meshgen.place(joints, 75.0, (6.0, -1.5, 0.9)).astype(np.float64), n_bones)
    return sd, lp, S


def receive_scene(n_paths=N_PATHS):
    """(sd, lp, S): tests/test_gpu_skin.py's _receive_scene restated: scenes.bus_receive with the bar in the bus's place, 2.5 times
    the size and turned broadside to the radar before the builder places it (yaw -20 degrees, at (10, 3, 1.7)); an I/Q launch"""
    n_bones = 3
    bv, bf, index, weight = meshgen.jointed_bar(n_bones, 8, 6, radius=0.4)
    joints = np.stack([np.arange(n_bones + 1, dtype=np.float64), np.zeros(n_bones + 1), np.zeros(n_bones + 1)], -1)
    local = lambda a: meshgen.place(np.asarray(a, np.float64) - [1.5, 0.0, 0.0], 90.0, (0.0, 0.0, 0.0), 2.5)
    sd, lp = scenes.bus_receive(n_paths=n_paths, mesh=(local(bv), bf))
    lp.mode = capi.BF_MODE_RECEIVE_IQ
    k = next(i for i, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH)
    S = Skin(k, _verts(sd, k), None, bf, index, weight, meshgen.place(local(joints), -20.0, (10.0, 3.0, 1.7)).astype(np.float64), n_bones)
    return sd, lp, S


def _m4(m):
    out = np.eye(4)
    out[:3] = np.asarray(m, np.float64).reshape(3, 4)
    return out


def bend(S, angles, axis=(0.2, 0.1, 1.0), root=None):
    """float32[n_bones, 3, 4]: bone 0 = `root` (identity), bone k = bone k - 1 after a turn by angles[k - 1] degrees about joint k"""
    m = np.eye(4) if root is None else _m4(root)
    bones = [m[:3].copy()]
    for k in range(1, S.n_bones):
        m = m @ _m4(motion.about(motion.rotation(axis, angles[k - 1]), S.joints[k]))
        bones.append(m[:3].copy())
    return np.ascontiguousarray(np.stack(bones), f32)


def posed(S, bones, dq=False):
    """float32[nv, 3]: the bar's vertices under `bones`"""
    fn = motion.apply_skin_dq if dq else motion.apply_skin
    return fn(S.rest, S.rest_n, S.index, S.weight, bones)[0]


def table(window=WINDOW, n_bins=N_BINS, sensor_lin=(0.0, 0.0, 0.0)):
    return capi.range_rate_bins(window, n_bins, sensor_lin=sensor_lin)


def still(sd):
    return np.stack([motion.twist() for _ in range(len(sd.shapes))])


def prim0(sd, k):
    """the oracle's primitive index of face 0 of shape k: rectangles count one, meshes their faces"""
    return sum(int(s.n_faces) if s.type == capi.BF_SHAPE_MESH else 1 for s in sd.shapes[:k])


def first_hits(sd, lp, twin=None, records=None, trace_sd=None):
    """(d float32[n, 3], p float32[n, 3], shape int64[n], prim int64[n], uv float32[n, 2]) of every path of launch `lp`: the
    direction of its primary ray, composed as range_rate_ref.first_points composes it, and the point, shape, primitive and
    barycentrics of its first intersection on `trace_sd` (default `sd`); shape -1 and zeros: none."""
    lib = oracle_lib.load()
    n = int(lp.n_paths)
    compose = OracleScene(twin if twin is not None else sd)
    sensor = (twin if twin is not None else sd).sensor
    pinhole = sensor.type in (capi.BF_SENSOR_PERSPECTIVE, capi.BF_SENSOR_RADIANCEMETER)
    film = bool(lp.spp and lp.film_width and lp.film_height)
    if film:
        assert sensor.crop_offset_x == 0 and sensor.crop_offset_y == 0, "first_hits composes films without a crop"
    W, H = (f32(lp.film_width), f32(lp.film_height)) if film else (f32(1), f32(1))
    rays = np.zeros((n, 8), f32)
    u = np.zeros(4, f32)
    for i in range(n):
        lib.bfo_sampler_floats(C.c_uint64(lp.seed + lp.path_offset + i), 4, u.ctypes.data_as(C.c_void_p))
        fx, fy = f32(u[0]), f32(u[1])
        ax, ay = (0.5, 0.5) if pinhole else (float(u[2]), float(u[3]))
        x, y = fx, fy
        if film:
            q = (lp.path_offset + i) // lp.spp
            x = (f32(q % lp.film_width) + fx) / W
            y = (f32(q // lp.film_width) + fy) / H
        r = compose.sensor_sample_ray(float(x), float(y), ax, ay)
        rays[i, 0:3], rays[i, 3], rays[i, 4:7], rays[i, 7] = r["o"], r["mint"], r["d"], np.inf
    tracer = OracleScene(trace_sd if trace_sd is not None else sd)
    t, prim, shape, uv = tracer.trace_closest(rays)
    hit = np.isfinite(t)
    if records is None:
        plain = copy_launch(lp, flags=lp.flags & ~capi.BF_FLAG_CLASSES)
        records = tracer.render(plain, records=True, threads=8)[1]
    valid = records["valid"] != 0
    assert np.array_equal(hit, valid), f"composed first hit differs from record.valid for {int((hit != valid).sum())} of {n} paths"
    p = np.zeros((n, 3), f32)
    for i in np.flatnonzero(hit):
        si = tracer.intersect_full(rays[i])
        assert si["t"] == t[i], (i, si["t"], t[i])
        p[i] = si["p"]
    return (rays[:, 4:7].copy(), p, np.where(hit, shape.astype(np.int64), -1), np.where(hit, prim.astype(np.int64), 0),
            np.where(hit[:, None], uv, f32(0)).astype(f32))


def hit_velocities(sd, shape, prim, uv, fields):
    """(U float32[n, 3], has bool[n]): the velocity interpolated at every path's first intersection, for the paths that meet a
    shape of `fields` ({shape: float32[n_vertices, 3]}, the world-space velocity of every vertex) first"""
    n = len(shape)
    U, has = np.zeros((n, 3), f32), np.zeros(n, bool)
    for k, V in fields.items():
        mine = np.flatnonzero(shape == int(k))
        if not len(mine):
            continue
        face = prim[mine] - prim0(sd, int(k))
        assert face.min() >= 0 and face.max() < int(sd.shapes[int(k)].n_faces), (k, face.min(), face.max())
        c = np.asarray(V, f32)[faces(sd, int(k))[face]]            # [hits, 3 corners, 3]
        U[mine] = capi.interpolate_velocity(uv[mine], c[:, 0], c[:, 1], c[:, 2])
        has[mine] = True
    return U, has


def classes(sd, lp, bins, twists, fields, twin=None, records=None, trace_sd=None):
    """int64[n]: the class of every path, and what it was computed from (d, p, shape, prim, uv, U, has)"""
    d, p, shape, prim, uv = first_hits(sd, lp, twin=twin, records=records, trace_sd=trace_sd)
    U, has = hit_velocities(trace_sd if trace_sd is not None else sd, shape, prim, uv, fields)
    return capi.range_rate_classes(d, p, shape, bins, twists, vertex_velocity=U, has_velocity=has), (d, p, shape, prim, uv, U, has)


def expected(sd, lp, bins, twists, fields, twin=None, singles=None, trace_sd=None):
    """first_hits + hit_velocities + range_rate_classes + class_ref.per_class of one launch: (Expected, oracle records, Addends of
    the plain launch).  `trace_sd`: the posed description the launch renders; `fields`: the velocity of every vertex of the shapes
    in BF_VELOCITY_VERTEX or BF_VELOCITY_DIFFERENCE."""
    plain = copy_launch(lp, flags=lp.flags & ~capi.BF_FLAG_CLASSES)
    on = trace_sd if trace_sd is not None else sd
    _, rec, _, add = OracleScene(on).render(plain, records=True, threads=8, addends=True)
    cls, _ = classes(sd, plain, bins, twists, fields, twin=twin, records=rec, trace_sd=trace_sd)
    return class_ref.per_class(on, plain, cls, capi.range_rate_n_classes(bins), addends=add, singles=singles), rec, add


@functools.lru_cache(maxsize=None)
def scene():
    return range_scene()


@functools.lru_cache(maxsize=None)
def _vertices(angles, dq=False):
    return posed(scene()[2], bend(scene()[2], list(angles)), dq)


@functools.lru_cache(maxsize=None)
def _described(angles, dq=False):
    sd, _, S = scene()
    return motion.deformed_description(sd, {S.k: _vertices(angles, dq)})


@functools.lru_cache(maxsize=None)
def _singles(angles, dq=False):
    return class_ref.single_path_hists(_described(angles, dq), scene()[1])


@functools.lru_cache(maxsize=None)
def bar_expected(angles, angles_prev, angles_next, dt=DT, dq=False):
    """Expected of the scene with the bar bent by `angles`, its field the difference of the poses `angles_prev` and `angles_next`
    over dt (None, None: at rest), under table() with every twist zero: shared by the tests that render that pose"""
    sd, lp, S = scene()
    V = np.zeros_like(S.rest) if angles_prev is None else capi.corner_velocities(_vertices(angles_prev, dq), _vertices(angles_next, dq), dt)
    return expected(sd, lp, table(), still(sd), {S.k: V}, singles=_singles(angles, dq), trace_sd=_described(angles, dq))
