"""Returns by direction of arrival (Scene.set_arrival_classes), the part that needs no GPU: the specification
capi.arrival_classes against hand-made vectors and against a scalar statement of the same roundings, csrc/bf_arrival.h compiled
as a host-only program against the specification bit for bit, the reference helper tests/arrival_ref.py on the scenes the GPU tests
use (every bin populated, the composed rays' hit / miss equal to the oracle's record.valid), and the new export."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from beifong_amd import capi, scenes
from tests import arrival_ref as ar
from tests import class_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "beifong_hip.h")
f32 = np.float32


def _below(x):
    return np.nextafter(f32(x), f32(-np.inf))


def _above(x):
    return np.nextafter(f32(x), f32(np.inf))


def _scalar_class(d, b):
    """the rule once more, one direction at a time in Python floats: every fp32 operation is the float64 operation rounded to
    fp32 (products of two fp32 are exact in float64; for sums, differences and quotients 53 >= 2 * 24 + 2 bits make the second
    rounding innocuous)"""
    r = lambda x: float(f32(x))
    d = [float(f32(x)) for x in d]

    def coordinate(axis, lo, hi, n):
        a = [float(f32(x)) for x in axis]
        u = r(r(r(d[0] * a[0]) + r(d[1] * a[1])) + r(d[2] * a[2]))
        s = r(float(n) / r(r(hi) - r(lo)))
        return r(r(u - r(lo)) * s)
    with np.errstate(all="ignore"):
        tu = coordinate(b.axis_u, b.u0, b.u1, b.n_u)
        tv = coordinate(b.axis_v, b.v0, b.v1, b.n_v)
    inside = tu >= 0.0 and tu < float(b.n_u) and tv >= 0.0 and tv < float(b.n_v)
    return int(tv) * b.n_u + int(tu) if inside else b.n_u * b.n_v


def _edge_directions():
    """directions whose u = d.y and v = d.z (axes y and z) sit on and next to the edges of the windows below, and the non-finite ones"""
    ys = [0.0, -0.0, 0.5, 0.6, -0.25, -1.0, 1.0, 0.3, 0.075, 0.15]
    ys = [f(y) for y in ys for f in (_below, f32, _above)]
    out = [(0.3, y, z) for y in ys for z in (0.0, -0.2, _below(-0.2), 0.4, _below(0.4), 0.1)]
    for bad in (np.nan, np.inf, -np.inf):
        out += [(bad, 0.1, 0.1), (0.1, bad, 0.1), (0.1, 0.1, bad), (bad, bad, bad)]
    return np.asarray(out, f32)


TABLES = {
    "narrow": ar.bins(8, 4, (0.0, 0.6, -0.2, 0.4)),
    "power_of_two": ar.bins(8, 4, (0.0, 0.5, -0.25, 0.25)),
    "asymmetric": ar.bins(5, 3, (-0.25, 0.6, 0.05, 0.4)),
    "one_row": ar.bins(32, 1, (-1.0, 1.0, -2.0, 2.0)),
    "whole_sphere": ar.bins(8, 4, (-1.0, 1.0, -1.0, 1.0)),
    "skew_axes": ar.bins(15, 17, (-0.7, 0.9, -0.33, 0.77), axis_u=(0.3, -0.8, 0.52), axis_v=(-0.61, 0.1, 0.7)),
    "largest": ar.bins(85, 3, (-1.0, 1.0, -1.0, 1.0)),
}


def test_specification_by_hand():
    b = TABLES["power_of_two"]                       # su = 16, sv = 8: tu = 16 u exactly
    cls = lambda y, z, bins=b: int(capi.arrival_classes([[0.9, y, z]], bins)[0])
    outside = 32
    assert capi.arrival_n_classes(b) == 33
    assert cls(0.0, -0.25) == 0                      # u exactly u0, v exactly v0: bin 0
    assert cls(-0.0, -0.25) == 0
    assert cls(_below(0.0), 0.0) == outside          # one ulp below u0
    assert cls(0.0, _below(-0.25)) == outside
    last = _below(0.5)                               # tu = 16 * (0.5 - ulp) = 8 - ulp: one ulp below n_u, the last bin
    assert f32(last) * f32(16) == _below(8.0) and cls(last, -0.25) == 7
    assert cls(0.5, -0.25) == outside                # tu == n_u
    assert cls(last, 0.2) == 31 and cls(last, 0.25) == outside
    # fl(v - v0) rounds before the comparison: 0.25 - ulp + 0.25 is a tie that rounds to 0.5, so tv = 4 = n_v although v < v1
    assert cls(0.0, _below(0.25)) == outside
    assert cls(0.0625, 0.0) == 2 * 8 + 1
    for bad in (np.nan, np.inf, -np.inf):            # a non-finite direction is outside, whichever component carries it
        for d in ([bad, 0.1, 0.1], [0.1, bad, 0.1], [0.1, 0.1, bad]):
            assert int(capi.arrival_classes([d], b)[0]) == outside, d
    # a window that is not symmetric about 0
    a = TABLES["asymmetric"]                         # u: 5 bins of 0.17 from -0.25; v: 3 bins from 0.05
    assert cls(-0.25, 0.05, a) == 0 and cls(_below(-0.25), 0.05, a) == 15 and cls(0.0, 0.06, a) == 1 and cls(0.59, 0.39, a) == 14
    assert cls(0.0, 0.0, a) == 15 and cls(0.0, 0.41, a) == 15
    # n_v = 1: the class is the u bin, v only decides inside / outside
    o = TABLES["one_row"]
    assert capi.arrival_n_classes(o) == 33
    assert [cls(y, 0.7, o) for y in (-1.0, -0.9375, 0.0, 0.9999)] == [0, 1, 16, 31] and cls(1.0, 0.7, o) == 32
    assert cls(0.0, 2.0, o) == 32 and cls(0.0, -2.0, o) == 16
    # where fl(u1 - ulp) * su rounds up to n_u the direction is outside although u < u1: the rule is on tu
    n = TABLES["narrow"]
    top = _below(0.6)
    tu = (top - f32(0.0)) * (f32(8) / (f32(0.6) - f32(0.0)))
    assert cls(top, 0.0, n) == (7 + 8 if tu < f32(8) else 32)


@pytest.mark.parametrize("name", sorted(TABLES))
def test_specification_against_scalar_roundings(name):
    b = TABLES[name]
    rng = np.random.default_rng(11)
    d = rng.normal(size=(2000, 3))
    d = np.concatenate([(d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32), _edge_directions()])
    got = capi.arrival_classes(d, b)
    assert got.dtype == np.int64 and got.min() >= 0 and got.max() <= b.n_u * b.n_v
    want = np.asarray([_scalar_class(x, b) for x in d])
    assert np.array_equal(got, want), (name, np.flatnonzero(got != want)[:8])
    if name != "one_row":
        assert len(np.unique(got)) >= min(20, b.n_u * b.n_v)      # the sample does exercise the bins


def test_arrival_header_is_plain_cxx(tmp_path):
    """bf_arrival.h compiles without HIP into a host-only program (tests/native/arrival_check.cpp) and gives the specification's
    classes, and the specification's scales, bit for bit"""
    exe = tmp_path / "arrival_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "native", "arrival_check.cpp")],
                   check=True)
    rng = np.random.default_rng(12)
    lines, want = [], []
    for name in sorted(TABLES):                       # 7 tables x 15000: about 1e5 random unit directions, and the edges with each
        b = TABLES[name]
        d = rng.normal(size=(15000, 3))
        d = np.concatenate([(d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32), _edge_directions()])
        dbits = d.view(np.uint32)
        words = np.asarray(list(b.axis_u) + list(b.axis_v) + [b.u0, b.u1, b.v0, b.v1], f32).view(np.uint32)
        lines.append(" ".join(str(int(w)) for w in words) + f" {b.n_u} {b.n_v} {len(d)}")
        lines += [f"{x} {y} {z}" for x, y, z in dbits.tolist()]
        su, sv = f32(b.n_u) / (f32(b.u1) - f32(b.u0)), f32(b.n_v) / (f32(b.v1) - f32(b.v0))
        want += [int(np.asarray(su, f32).view(np.uint32)), int(np.asarray(sv, f32).view(np.uint32))]
        want += capi.arrival_classes(d, b).tolist()
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    got = [int(x) for x in out.split()]
    assert len(got) == len(want) and got == want


def _population(cls, b):
    pop = np.bincount(cls, minlength=capi.arrival_n_classes(b))
    return pop[:-1], int(pop[-1])


@pytest.mark.parametrize("mode", [capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ], ids=["raw", "iq"])
def test_directions_receive_through_the_twin(mode):
    sd, lp = class_ref.receive_scene(4096)
    lp.mode = mode
    d = ar.directions(sd, lp, twin=class_ref.fluxmeter_twin(class_ref.receive_scene))
    assert d.shape == (4096, 3) and d.dtype == f32 and np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-5)
    inside, outside = _population(capi.arrival_classes(d, TABLES["narrow"]), TABLES["narrow"])
    assert inside.min() >= 1 and outside > 0 and inside.sum() + outside == 4096, (inside, outside)
    inside, outside = _population(capi.arrival_classes(d, TABLES["whole_sphere"]), TABLES["whole_sphere"])
    assert inside.min() >= 1 and outside == 0, (inside, outside)


def test_directions_film():
    sd, lp = class_ref.film_scene()
    b = ar.bins(6, 4, (-0.3, 0.3, -0.2, 0.2))
    d = ar.directions(sd, lp)
    inside, outside = _population(capi.arrival_classes(d, b), b)
    assert inside.min() >= 1 and outside > 0 and inside.sum() + outside == int(lp.n_paths), (inside, outside)


def test_bins_for_the_sensors_own_axes():
    """arrival_bins_for: the normalised tangent columns of the sensor's to_world, float64 rounded once"""
    sd, _ = class_ref.receive_scene(16)
    b = capi.arrival_bins_for(sd, 32, 1, (-1.0, 1.0, -2.0, 2.0))
    m = np.asarray(list(sd.shapes[int(sd.sensor.shape)].to_world), np.float64).reshape(4, 4)
    for axis, k in ((b.axis_u, 0), (b.axis_v, 1)):
        want = (m[:3, k] / np.linalg.norm(m[:3, k])).astype(f32)
        assert np.array_equal(np.asarray(list(axis), f32), want) and abs(float(np.linalg.norm(want.astype(np.float64))) - 1.0) < 1e-6
    assert (b.n_u, b.n_v, b.u0, b.u1, b.v0, b.v1) == (32, 1, -1.0, 1.0, -2.0, 2.0)
    fd, _ = class_ref.film_scene()
    c = capi.arrival_bins_for(fd, 6, 4, (-0.3, 0.3, -0.2, 0.2))
    cam = np.asarray(list(fd.sensor.to_world), np.float64).reshape(4, 4)
    assert np.array_equal(np.asarray(list(c.axis_u), f32), (cam[:3, 0] / np.linalg.norm(cam[:3, 0])).astype(f32))
    # the camera's own axes: its boresight has direction cosines 0, 0
    z = (cam[:3, 2] / np.linalg.norm(cam[:3, 2])).astype(f32)
    mid = capi.arrival_bins_for(fd, 5, 3, (-0.5, 0.5, -0.3, 0.3))
    assert int(capi.arrival_classes([z], mid)[0]) == 1 * 5 + 2


def test_library_exports_the_arrival_entry():
    lib = C.CDLL(capi.LIB_PATH)
    assert "bf_scene_set_arrival_classes" in capi.EXPORTED_SYMBOLS
    getattr(lib, "bf_scene_set_arrival_classes")          # AttributeError: not exported
    text = open(HEADER).read()
    assert re.search(r"#define BF_ABI_VERSION 5\b", text) and capi.BF_ABI_VERSION == 5      # no struct or signature changed
    assert "bf_scene_set_arrival_classes(bf_scene *scene, const bf_arrival_bins *bins, void *stream)" in text
    assert C.sizeof(capi.bf_arrival_bins) == 48
    lib = capi.load_library()
    b = TABLES["narrow"]
    assert lib.bf_scene_set_arrival_classes(None, C.byref(b), None) == capi.BF_ERR_INVALID
    assert b"bf_scene_set_arrival_classes" in (lib.bf_last_error() or b"")
