"""Per-vertex velocities under the range-rate table (Scene.set_velocity_mode), without a GPU: the numpy specification
(capi.corner_velocities, capi.interpolate_velocity, capi.range_rate_classes with vertex_velocity=) against a scalar restatement and
hand-made vectors, csrc/bf_velocity.h compiled as a plain C++ program against the specification bit for bit, the new entries in the
header, the binding and the built library, and the populations of the bins on the oracle for the scene tests/test_gpu_velocity.py
renders (tests/velocity_ref.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from beifong_amd import capi, motion
from tests import velocity_ref as vr

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["bf_scene_set_velocity_mode", "bf_scene_get_velocity_mode", "bf_scene_set_vertex_velocities", "bf_scene_set_vertex_velocities_device"]


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _same_bits(a, b):
    """bit-equal, NaNs of any payload equal to each other"""
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _scalar_interpolate(u, v, v0, v1, v2):
    """the rule of include/beifong_hip.h, one float32 operation at a time"""
    with np.errstate(all="ignore"):
        b0 = f32(f32(f32(1) - f32(u)) - f32(v))
        return [f32(f32(f32(b0 * f32(v0[c])) + f32(f32(u) * f32(v1[c]))) + f32(f32(v) * f32(v2[c]))) for c in range(3)]


def _scalar_rate(d, p, tw, sl, U):
    with np.errstate(all="ignore"):
        lin, ang, piv = tw[0:3], tw[3:6], tw[6:9]
        q = [f32(f32(p[c]) - f32(piv[c])) for c in range(3)]
        cr = [f32(f32(ang[(c + 1) % 3] * q[(c + 2) % 3]) - f32(ang[(c + 2) % 3] * q[(c + 1) % 3])) for c in range(3)]
        if U is None:
            w = [f32(f32(lin[c] + cr[c]) - f32(sl[c])) for c in range(3)]
        else:
            w = [f32(f32(f32(lin[c] + cr[c]) + f32(U[c])) - f32(sl[c])) for c in range(3)]
        return f32(f32(f32(d[0] * w[0]) + f32(d[1] * w[1])) + f32(d[2] * w[2]))


def _random_cases(rng, n):
    prev = rng.uniform(-20, 20, (n, 3, 3)).astype(f32)
    nxt = (prev + rng.normal(0, 0.02, (n, 3, 3))).astype(f32)
    dt = f32(2.0) ** rng.integers(-9, -3, n).astype(f32) * rng.uniform(1, 2, n).astype(f32)
    uv = rng.dirichlet([1, 1, 1], n)[:, 1:].astype(f32)
    tw = np.concatenate([rng.normal(0, 2, (n, 3)), rng.normal(0, 1, (n, 3)), rng.uniform(-10, 10, (n, 3))], 1).astype(f32)
    sl = rng.normal(0, 3, (n, 3)).astype(f32)
    return prev, nxt, dt, uv, tw, sl


def _edge_cases():
    """hand-made vectors behind the random ones: the corners of the triangle, a uniform field, a zero field, -0, NaN and inf in the
    field, a difference in the subnormals, a quotient that overflows"""
    nan, inf, tiny = f32("nan"), f32("inf"), f32(1e-45)
    one = np.zeros((3, 3), f32)
    rows = []
    base = dict(prev=one.copy(), nxt=np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], f32) / 64, dt=f32(1 / 64), uv=(0.25, 0.5),
                tw=np.array([0.5, -0.25, 0, 0, 0, 0.75, 1, 2, 3], f32), sl=np.array([1, 0, 0], f32))
    for uv in ((0, 0), (1, 0), (0, 1), (0.25, 0.5), (1 / 3, 1 / 3)):
        rows.append(dict(base, uv=uv))
    rows.append(dict(base, nxt=np.tile(np.array([0.5, -0.125, 0.25], f32) / 64, (3, 1))))      # a uniform field
    rows.append(dict(base, nxt=one.copy()))                                                      # a zero field
    rows.append(dict(base, nxt=-one, tw=np.zeros(9, f32), sl=np.zeros(3, f32)))                  # -0 everywhere
    for bad in (nan, inf, -inf):
        n = base["nxt"].copy()
        n[1, 2] = bad
        rows.append(dict(base, nxt=n))
    rows.append(dict(base, prev=np.full((3, 3), 1e-38, f32), nxt=np.full((3, 3), f32(1e-38) + 4 * tiny, f32), dt=f32(1.0)))      # subnormal difference
    rows.append(dict(base, prev=np.full((3, 3), 1e-38, f32), nxt=np.full((3, 3), f32(1e-38) + 4 * tiny, f32), dt=f32(3.0)))      # ... and quotient
    rows.append(dict(base, nxt=np.full((3, 3), 1e30, f32), dt=f32(1e-30)))                       # the quotient overflows
    keys = ("prev", "nxt", "dt", "uv", "tw", "sl")
    return tuple(np.stack([np.asarray(r[k], f32) for r in rows]) for k in keys)


def _spec(prev, nxt, dt, uv, tw, sl, bins):
    """(V [n, 3, 3], U [n, 3], rr [n], class [n]) of the specification, the point and direction as tests/native/velocity_check.cpp
    takes them from the same numbers"""
    n = len(prev)
    V = capi.corner_velocities(prev, nxt, dt.reshape(n, 1, 1))
    U = capi.interpolate_velocity(uv, V[:, 0], V[:, 1], V[:, 2])
    p = np.stack([nxt[:, 0, 0], nxt[:, 1, 1], nxt[:, 2, 2]], 1)
    d = np.stack([tw[:, 3], tw[:, 1], tw[:, 8]], 1)
    rr = np.empty(n, f32)
    cls = np.empty(n, np.int64)
    for i in range(n):      # (one shape per case: the table is that shape's twist, the radar's velocity the case's)
        b = capi.range_rate_bins((bins.r0, bins.r1), bins.n_bins, sensor_lin=sl[i])
        rr[i] = capi.range_rates(d[i:i + 1], p[i:i + 1], [0], b, tw[i:i + 1], U[i:i + 1], [True])[0]
        cls[i] = capi.range_rate_classes(d[i:i + 1], p[i:i + 1], [0], b, tw[i:i + 1], U[i:i + 1], [True])[0]
    return V, U, rr, cls, p, d


def test_specification_by_hand():
    V0, V1, V2 = (np.array([x], f32) for x in ([1.5, -2.25, 0.1], [0.3, 7.0, -1e-3], [-4.0, 0.7, 2.5]))
    assert _same_bits(capi.interpolate_velocity([[0, 0]], V0, V1, V2), V0)
    assert _same_bits(capi.interpolate_velocity([[1, 0]], V0, V1, V2), V1)
    assert _same_bits(capi.interpolate_velocity([[0, 1]], V0, V1, V2), V2)
    # a uniform field: itself where the three weights are exact binary fractions, the stated roundings of it elsewhere
    assert _same_bits(capi.interpolate_velocity([[0.25, 0.5]], V0, V0, V0), V0)
    third = capi.interpolate_velocity([[f32(1 / 3), f32(1 / 3)]], V0, V0, V0)
    assert _same_bits(third, [_scalar_interpolate(f32(1 / 3), f32(1 / 3), V0[0], V0[0], V0[0])])
    assert np.allclose(third, V0, rtol=4 * 2.0 ** -24, atol=0)
    # a zero field under a twist: the class of BF_VELOCITY_TWIST, whatever the hit
    b = capi.range_rate_bins((-6.0, -2.0), 8, sensor_lin=(4.0, 0.0, 0.0))
    rng = np.random.default_rng(5)
    d = rng.normal(size=(64, 3)).astype(f32)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(f32)
    p = rng.uniform(-10, 10, (64, 3)).astype(f32)
    tw = [motion.twist(lin=(-2.0, -0.5, 0.0), ang=(0.0, 0.0, 0.8), pivot=(10.0, 3.0, 1.7))]
    shape = np.zeros(64, np.int64)
    plain = capi.range_rate_classes(d, p, shape, b, tw)
    assert len(set(plain.tolist())) > 3
    assert np.array_equal(capi.range_rate_classes(d, p, shape, b, tw, vertex_velocity=np.zeros((64, 3), f32)), plain)
    # ... and has_velocity selects the paths the field applies to
    U = np.tile(f32([3.0, 0.0, 0.0]), (64, 1))
    has = np.arange(64) % 2 == 0
    mixed = capi.range_rate_classes(d, p, shape, b, tw, vertex_velocity=U, has_velocity=has)
    moved = capi.range_rate_classes(d, p, shape, b, tw, vertex_velocity=U)
    assert np.array_equal(mixed[~has], plain[~has]) and np.array_equal(mixed[has], moved[has]) and not np.array_equal(moved, plain)
    # -0, NaN and inf in the field: outside the window [-1, 0) (t = n_bins for a rate of +-0; a NaN compares false)
    w = capi.range_rate_bins((-1.0, 0.0), 8)
    rest = [motion.twist()]
    for bad in (-0.0, np.nan, np.inf, -np.inf):
        got = capi.range_rate_classes([[0.6, 0.0, 0.8]], [[1, 2, 3]], [0], w, rest, vertex_velocity=[[bad, 0.0, 0.0]])
        assert got.tolist() == [8], (bad, got)
    assert capi.range_rate_classes([[0.6, 0.0, 0.8]], [[1, 2, 3]], [0], w, rest, vertex_velocity=[[-0.5, 0.0, 0.0]]).tolist() == [5]
    # the difference: a result in the subnormals, and a quotient that overflows
    tiny = f32(1e-45)
    a, c = f32(1e-38), f32(1e-38) + 4 * tiny
    v = capi.corner_velocities([a], [c], 1.0)
    assert v.dtype == f32 and v[0] == 4 * tiny and 0 < v[0] < np.finfo(f32).tiny
    assert capi.corner_velocities([a], [c], 3.0)[0] == f32(f32(c - a) / f32(3.0)) == tiny      # 4/3 of the smallest subnormal rounds to it
    assert np.isposinf(capi.corner_velocities([0.0], [1e30], 1e-30)[0]) and np.isneginf(capi.corner_velocities([1e30], [0.0], 1e-30)[0])
    assert _same_bits(motion.vertex_velocities([[0.0, 1.0, 2.0]], [[0.5, 1.0, 1.0]], 1 / 64), [[32.0, 0.0, -64.0]])


def test_specification_against_scalar_roundings():
    rng = np.random.default_rng(31)
    prev, nxt, dt, uv, tw, sl = (np.concatenate([a, b]) for a, b in zip(_random_cases(rng, 1500), _edge_cases()))
    b = capi.range_rate_bins((-6.0, 2.0), 16)
    V, U, rr, cls, p, d = _spec(prev, nxt, dt, uv, tw, sl, b)
    with np.errstate(all="ignore"):
        for i in range(len(prev)):
            Vi = [[f32(f32(nxt[i, j, c] - prev[i, j, c]) / dt[i]) for c in range(3)] for j in range(3)]
            assert _same_bits(V[i], Vi), i
            Ui = _scalar_interpolate(uv[i, 0], uv[i, 1], Vi[0], Vi[1], Vi[2])
            assert _same_bits(U[i], Ui), i
            assert _same_bits([rr[i]], [_scalar_rate(d[i], p[i], tw[i], sl[i], Ui)]), i
            # has_velocity false: the present expression, unchanged
            bi = capi.range_rate_bins((b.r0, b.r1), b.n_bins, sensor_lin=sl[i])
            off = capi.range_rates(d[i:i + 1], p[i:i + 1], [0], bi, tw[i:i + 1], U[i:i + 1], [False])
            assert _same_bits(off, [_scalar_rate(d[i], p[i], tw[i], sl[i], None)]) and _same_bits(off, capi.range_rates(d[i:i + 1], p[i:i + 1], [0], bi, tw[i:i + 1]))
    assert len(set(cls.tolist())) == 17      # every bin and the class outside


def test_velocity_header_is_plain_cxx(tmp_path):
    """bf_velocity.h compiles without HIP into a host-only program (tests/native/velocity_check.cpp) and gives the specification's
    corner velocities, interpolated velocities, rates and classes, bit for bit"""
    exe = tmp_path / "velocity_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "native", "velocity_check.cpp")],
                   check=True)
    rng = np.random.default_rng(32)
    prev, nxt, dt, uv, tw, sl = (np.concatenate([a, b]) for a, b in zip(_random_cases(rng, 10000), _edge_cases()))
    n = len(prev)
    b = capi.range_rate_bins((-6.0, 2.0), 16)
    table = np.concatenate([prev.reshape(n, 9), nxt.reshape(n, 9), dt.reshape(n, 1), uv, tw, sl], 1)
    assert table.shape == (n, 33) and table.dtype == f32
    lines = [str(n)] + [" ".join(str(int(x)) for x in row) for row in _bits(table)]
    lines.append(f"{int(_bits([b.r0])[0])} {int(_bits([b.r1])[0])} {int(b.n_bins)}")
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    got = np.array([int(x) for x in out.split()], np.uint32).reshape(n, 14)
    V, U, rr, cls, _, _ = _spec(prev, nxt, dt, uv, tw, sl, b)
    assert _same_bits(got[:, 0:9].view(f32), V.reshape(n, 9))
    assert _same_bits(got[:, 9:12].view(f32), U)
    assert _same_bits(got[:, 12].view(f32), rr)
    assert np.array_equal(got[:, 13].astype(np.int64), cls)
    assert np.isnan(rr).any() and np.isinf(V).any() and len(set(cls.tolist())) == 17


def test_entries_are_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "beifong_hip.h")) as f:
        header = f.read()
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert re.search(rf"\bbf_status {name}\(", header), name
        assert name in capi.EXPORTED_SYMBOLS
        getattr(lib, name)          # AttributeError: not exported
    assert re.search(r"BF_VELOCITY_TWIST = 0, BF_VELOCITY_VERTEX = 1, BF_VELOCITY_DIFFERENCE = 2", header)
    assert (capi.BF_VELOCITY_TWIST, capi.BF_VELOCITY_VERTEX, capi.BF_VELOCITY_DIFFERENCE) == (0, 1, 2)
    assert capi.BF_ABI_VERSION == 5 and re.search(r"#define BF_ABI_VERSION 5\b", header)


def test_populations_on_the_oracle():
    """the bar bent by POSES[0], its field the difference to POSES[1] over 1/64 s: every bin of [-1, 0) m/s and the class outside are
    populated by the bar's first hits, the rates outside lie on both sides of the window, and everything else in the scene, at rest
    under zero twists, has the rate 0: outside"""
    sd, lp, S = vr.scene()
    assert len(S.faces) == 304 and int(sd.shapes[S.k - 1].n_faces) == 976 and vr.prim0(sd, S.k) == vr.BAR_PRIM0
    a0, a1 = tuple(vr.POSES[0]), tuple(vr.POSES[1])
    V = capi.corner_velocities(vr._vertices(a0), vr._vertices(a1), vr.DT)
    cls, (d, p, shape, prim, uv, U, has) = vr.classes(sd, lp, vr.table(), vr.still(sd), {S.k: V}, trace_sd=vr._described(a0))
    bar = shape == S.k
    assert int(bar.sum()) == vr.BAR_HITS and np.array_equal(has, bar)
    pop = np.bincount(cls[bar], minlength=vr.N_BINS + 2)
    assert pop[:vr.N_BINS].min() >= 1 and pop[vr.N_BINS] > 0 and pop[vr.N_BINS + 1] == 0, pop
    assert (pop[:vr.N_BINS].tolist(), int(pop[vr.N_BINS])) == vr.BAR_POPULATION, pop
    rr = capi.range_rates(d, p, shape, vr.table(), vr.still(sd), U, has)[bar]
    assert (rr < vr.WINDOW[0]).sum() > 0 and (rr >= vr.WINDOW[1]).sum() > 0
    # the barycentric convention: the same three roundings applied to the posed corners give the oracle's point exactly
    c = vr._vertices(a0)[vr.faces(sd, S.k)[prim[bar] - vr.BAR_PRIM0]]
    assert _same_bits(capi.interpolate_velocity(uv[bar], c[:, 0], c[:, 1], c[:, 2]), p[bar])
    # whatever else a path meets first is at rest: rate 0, the class outside; a miss has its own
    rest = capi.range_rates(d, p, shape, vr.table(), vr.still(sd), U, has)[(shape >= 0) & ~bar]
    assert len(rest) > 1000 and not rest.any()
    assert np.array_equal(cls[(shape >= 0) & ~bar], np.full(len(rest), vr.N_BINS)) and np.all(cls[shape < 0] == vr.N_BINS + 1)
