"""Returns by range rate (Scene.set_range_rate_classes), the part that needs no GPU: the specification
capi.range_rate_classes against hand-made vectors and against a scalar statement of the same roundings, csrc/bf_range_rate.h
compiled as a host-only program against the specification bit for bit, the reference helper tests/range_rate_ref.py on the scenes
the GPU tests use (every bin of every table populated, the composed rays' hit / miss equal to the oracle's record.valid), and the
new export."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

from beifong_amd import capi, motion, scenes
from tests import class_ref
from tests import range_rate_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "beifong_hip.h")
f32 = np.float32

SENSOR_LIN, POPULATIONS, table, twists = rr.SENSOR_LIN, rr.POPULATIONS, rr.table, rr.twists      # what the GPU tests install


def _below(x):
    return np.nextafter(f32(x), f32(-np.inf))


def _above(x):
    return np.nextafter(f32(x), f32(np.inf))


def _scalar(d, p, tw, b):
    """the rule once more, one path at a time in Python floats: every fp32 operation is the float64 operation rounded to fp32
    (products of two fp32 are exact in float64; for sums, differences and quotients 53 >= 2 * 24 + 2 bits make the second
    rounding innocuous).  Returns (rr, sr, class of a hit)."""
    r = lambda x: float(f32(x))
    d, p = [r(x) for x in d], [r(x) for x in p]
    lin, ang, pivot = ([r(x) for x in tw[k:k + 3]] for k in (0, 3, 6))
    sl = [r(x) for x in b.sensor_lin]
    with np.errstate(all="ignore"):
        q = [r(p[k] - pivot[k]) for k in range(3)]
        c = [r(r(ang[1] * q[2]) - r(ang[2] * q[1])), r(r(ang[2] * q[0]) - r(ang[0] * q[2])), r(r(ang[0] * q[1]) - r(ang[1] * q[0]))]
        w = [r(r(lin[k] + c[k]) - sl[k]) for k in range(3)]
        rate = r(r(r(d[0] * w[0]) + r(d[1] * w[1])) + r(d[2] * w[2]))
        sr = r(float(b.n_bins) / r(r(b.r1) - r(b.r0)))
        t = r(r(rate - r(b.r0)) * sr)
    return rate, sr, (int(t) if 0.0 <= t < float(b.n_bins) else int(b.n_bins))


def _one(d, p, tw, b, shape=0):
    return int(capi.range_rate_classes([d], [p], [shape], b, [tw])[0])


def test_specification_by_hand():
    rest, x = motion.twist(), (1.0, 0.0, 0.0)
    # every twist zero over [0, r1): every hit lands in bin 0, whatever the ray; rr is -0 where d has a negative component
    b = capi.range_rate_bins((0.0, 3.0), 5)
    assert capi.range_rate_n_classes(b) == 7
    rng = np.random.default_rng(3)
    d = rng.normal(size=(64, 3)).astype(f32)
    p = (10 * rng.normal(size=(64, 3))).astype(f32)
    rates = capi.range_rates(d, p, np.zeros(64, int), b, [rest])
    assert np.all(rates == 0) and np.signbit(rates).any() and not np.signbit(rates).all()
    assert np.all(capi.range_rate_classes(d, p, np.zeros(64, int), b, [rest]) == 0)
    back = (-1.0, -1.0, -1.0)                         # three products -0: rr = -0, t = fl(fl(-0 - 0) * sr) = -0, and -0 >= 0
    assert _one(back, (1.0, 2.0, 3.0), rest, b) == 0 and np.signbit(capi.range_rates([back], [(1.0, 2.0, 3.0)], [0], b, [rest])[0])
    # ... and over [r0, 0) every hit lands outside: t = fl(fl(0 - r0) * sr) = n_bins
    for window, n in (((-4.0, 0.0), 4), ((-3.0, 0.0), 5), ((-0.7, 0.0), 11)):
        b = capi.range_rate_bins(window, n)
        assert (f32(0) - f32(window[0])) * (f32(n) / (f32(0) - f32(window[0]))) == f32(n)
        assert np.all(capi.range_rate_classes(d, p, np.zeros(64, int), b, [rest]) == n)
    # rr exactly r0 (bin 0) and one ulp below (outside); a pure translation along x seen along x has rr = v
    b = capi.range_rate_bins((-6.0, 2.0), 8)          # sr = 1: t = rr + 6
    along = lambda v: motion.twist(lin=(v, 0.0, 0.0))
    assert _one(x, (0, 0, 0), along(-6.0), b) == 0 and _one(x, (0, 0, 0), along(_below(-6.0)), b) == 8
    assert _one(x, (0, 0, 0), along(_above(-6.0)), b) == 0 and _one(x, (0, 0, 0), along(-5.0), b) == 1
    # t one ulp below n_bins (the last bin) and equal to it (outside)
    assert _one(x, (0, 0, 0), along(1.5), b) == 7 and _one(x, (0, 0, 0), along(2.0), b) == 8
    b16 = capi.range_rate_bins((0.0, 0.5), 8)         # sr = 16
    last = _below(0.5)
    assert f32(last) * f32(16) == _below(8.0) and _one(x, (0, 0, 0), along(last), b16) == 7 and _one(x, (0, 0, 0), along(0.5), b16) == 8
    # fl(rr - r0) rounds before the comparison: fl(2 - ulp + 6) = 8 = n_bins, so that rate is outside although rr < r1: the rule is on t
    assert f32(_below(2.0)) - f32(-6.0) == f32(8) and _one(x, (0, 0, 0), along(_below(2.0)), b) == 8
    # a pure translation along x: rr == fl(d.x v), the lever arm does not enter
    dd = np.asarray([(0.3, 0.4, 0.5), (-0.7, 0.1, 0.2), (1.0, -1.0, 1.0)], f32)
    for v in (3.3, -12.7, 1e-3):
        got = capi.range_rates(dd, p[:3], [0, 0, 0], b, [along(v)])
        assert np.array_equal(got, dd[:, 0] * f32(v))
    # the radar's own velocity enters with the other sign: a still scene from a radar driving along +x closes at d.x v
    bs = capi.range_rate_bins((-6.0, 2.0), 8, sensor_lin=(3.3, 0.0, 0.0))
    assert np.array_equal(capi.range_rates(dd, p[:3], [0, 0, 0], bs, [rest]), dd[:, 0] * f32(-3.3))
    # a pure spin about z through the pivot: the velocity of p = pivot + (L, 0, 0) is (0, w L, 0): rr along y is linear in L
    spin = motion.twist(ang=(0.0, 0.0, 0.75), pivot=(10.0, 3.0, 1.7))
    arms = np.asarray([0.0, 0.5, 1.0, 2.0, -4.0, 6.5], f32)
    pts = np.stack([f32(10.0) + arms, np.full(6, 3.0, f32), np.full(6, 1.7, f32)], -1)
    got = capi.range_rates(np.tile(np.asarray([(0.0, 1.0, 0.0)], f32), (6, 1)), pts, np.zeros(6, int), b, [spin])
    assert np.array_equal(got, f32(0.75) * arms)
    assert capi.range_rate_classes(np.tile(np.asarray([(0.0, 1.0, 0.0)], f32), (6, 1)), pts, np.zeros(6, int), b, [spin]).tolist() == [6, 6, 6, 7, 3, 8]
    # ... and nothing along the arm or along the axis
    for axis in ((1.0, 0.0, 0.0), (0.0, 0.0, 1.0)):
        assert np.all(capi.range_rates(np.tile(np.asarray([axis], f32), (6, 1)), pts, np.zeros(6, int), b, [spin]) == 0)
    # an overflowing ang x q: inf (or inf - inf, a NaN) is outside
    wild = motion.twist(ang=(0.0, 3e38, 3e38), pivot=(0.0, 0.0, 0.0))
    for pt in ((1e10, 1e10, 1e10), (0.0, 1e10, 0.0), (1e10, -1e10, 1e10)):
        for ray in ((1.0, 0.0, 0.0), (0.6, 0.0, 0.8), (0.0, -1.0, 0.0)):
            assert not np.isfinite(capi.range_rates([ray], [pt], [0], b, [wild])[0]) and _one(ray, pt, wild, b) == 8
    # a miss: n_bins + 1, whatever d and p are; the row of the shape is not looked at
    assert capi.range_rate_classes(dd, p[:3], [-1, 0, -1], b, [along(-5.0)]).tolist() == [9, 8, 9]      # (-0.7 * -5 + 6 = 9.5: outside)
    assert capi.range_rate_classes([(np.nan, 0, 0)], [(np.nan, 0, 0)], [-1], b, [wild]).tolist() == [9]
    # the second shape's row is the second shape's
    two = [along(-5.0), along(1.5)]
    assert capi.range_rate_classes([x, x], [(0, 0, 0)] * 2, [0, 1], b, two).tolist() == [1, 7]
    # bin centres
    assert np.array_equal(capi.range_rate_centres(b), -6.0 + (np.arange(8) + 0.5)) and capi.range_rate_centres(b).dtype == np.float64
    assert np.allclose(capi.range_rate_centres(capi.range_rate_bins((-25.0, 25.0), 64)), -25.0 + (np.arange(64) + 0.5) * 0.78125, rtol=0, atol=1e-12)
    # motion.twist
    assert np.array_equal(motion.twist(), np.zeros(9, f32)) and motion.twist((1, 2, 3), (4, 5, 6), (7, 8, 9)).tolist() == list(range(1, 10))


def _random_cases(rng, n):
    """random rays, points and twists of the size the scenes have, and the edge vectors with them"""
    d = rng.normal(size=(n, 3))
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32)
    p = (rng.normal(size=(n, 3)) * (8.0, 8.0, 2.0)).astype(f32)
    tw = np.concatenate([rng.normal(size=(n, 3)) * 5.0, rng.normal(size=(n, 3)), rng.normal(size=(n, 3)) * 6.0], 1).astype(f32)
    edge_d, edge_p, edge_tw = [], [], []
    for v in (-6.0, _below(-6.0), _above(-6.0), 2.0, _below(2.0), 0.0, -0.0, -2.0, _below(-2.0), 0.5, _below(0.5), np.inf, -np.inf, np.nan, 3e38):
        for ray in ((1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (0.6, 0.0, 0.8)):
            edge_d.append(ray), edge_p.append((1.0, 2.0, 3.0)), edge_tw.append(motion.twist(lin=(v, 0.0, 0.0)))
    edge_d.append((0.0, 1.0, 0.0)), edge_p.append((1e10, 1e10, 1e10)), edge_tw.append(motion.twist(ang=(0.0, 3e38, 3e38)))
    edge_d.append((0.0, 1.0, 0.0)), edge_p.append((12.0, 3.0, 1.7)), edge_tw.append(motion.twist(ang=(0.0, 0.0, 0.75), pivot=(10.0, 3.0, 1.7)))
    return (np.concatenate([d, np.asarray(edge_d, f32)]), np.concatenate([p, np.asarray(edge_p, f32)]),
            np.concatenate([tw, np.asarray(edge_tw, f32)]))


SPEC_TABLES = {
    "narrow": table("narrow"),
    "wide": table("wide"),
    "still_radar": capi.range_rate_bins((-6.0, 2.0), 8),
    "sixteen_per_unit": capi.range_rate_bins((0.0, 0.5), 8),
    "odd": capi.range_rate_bins((-3.3, 7.1), 13, sensor_lin=(0.3, -1.7, 2.9)),
    "one_bin": capi.range_rate_bins((-1e30, 1e30), 1, sensor_lin=SENSOR_LIN),
    "largest": capi.range_rate_bins((-25.0, 25.0), 254, sensor_lin=(1.0, 1.0, 1.0)),
}


@pytest.mark.parametrize("name", sorted(SPEC_TABLES))
def test_specification_against_scalar_roundings(name):
    b = SPEC_TABLES[name]
    d, p, tw = _random_cases(np.random.default_rng(21), 2000)
    n = len(d)
    got = capi.range_rate_classes(d, p, np.arange(n), b, tw)          # path i meets shape i: every path its own row
    rates = capi.range_rates(d, p, np.arange(n), b, tw)
    assert got.dtype == np.int64 and rates.dtype == f32 and got.min() >= 0 and got.max() <= b.n_bins
    want = [_scalar(d[i], p[i], tw[i], b) for i in range(n)]
    assert np.array_equal(got, np.asarray([w[2] for w in want])), (name, np.flatnonzero(got != np.asarray([w[2] for w in want]))[:8])
    wr = np.asarray([w[0] for w in want])
    assert np.array_equal(np.isnan(rates), np.isnan(wr)) and np.array_equal(rates[~np.isnan(wr)].astype(np.float64), wr[~np.isnan(wr)])
    if name not in ("one_bin",):
        assert len(np.unique(got)) >= min(8, b.n_bins)      # the sample does exercise the bins
    miss = capi.range_rate_classes(d, p, np.full(n, -1), b, tw)
    assert np.all(miss == b.n_bins + 1)


def test_range_rate_header_is_plain_cxx(tmp_path):
    """bf_range_rate.h compiles without HIP into a host-only program (tests/native/range_rate_check.cpp) and gives the
    specification's rates, classes and scale, bit for bit"""
    exe = tmp_path / "range_rate_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "native", "range_rate_check.cpp")],
                   check=True)
    rng = np.random.default_rng(22)
    bits = lambda a: np.asarray(a, f32).view(np.uint32)
    lines, want = [], []
    for name in sorted(SPEC_TABLES):                  # 7 tables x 15000 random paths, and the edges with each
        b = SPEC_TABLES[name]
        d, p, tw = _random_cases(rng, 15000)
        n = len(d)
        head = bits(list(b.sensor_lin) + [b.r0, b.r1])
        lines.append(" ".join(str(int(w)) for w in head) + f" {b.n_bins} {n}")
        rows = np.concatenate([bits(tw), bits(p), bits(d)], 1)
        lines += [" ".join(map(str, row)) for row in rows.tolist()]
        sr = f32(b.n_bins) / (f32(b.r1) - f32(b.r0))
        want.append((int(bits(sr)), capi.range_rates(d, p, np.arange(n), b, tw), capi.range_rate_classes(d, p, np.arange(n), b, tw)))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    got = [int(x) for x in out.split()]
    at = 0
    for sr, rates, cls in want:
        assert got[at] == sr
        g = np.asarray(got[at + 1:at + 1 + 2 * len(cls)], np.int64).reshape(-1, 2)
        at += 1 + 2 * len(cls)
        assert np.array_equal(g[:, 1], cls)
        grates = g[:, 0].astype(np.uint32).view(f32)
        nan = np.isnan(rates)
        assert np.array_equal(np.isnan(grates), nan) and np.array_equal(g[~nan, 0].astype(np.uint32), rates[~nan].view(np.uint32))      # (-0 as -0)
    assert at == len(got)


def _population(cls, b):
    """(paths per bin, paths outside, paths that miss)"""
    pop = np.bincount(cls, minlength=capi.range_rate_n_classes(b))
    return pop[:-2], int(pop[-2]), int(pop[-1])


@functools.lru_cache(maxsize=None)
def _receive_points(mode):
    sd, lp = class_ref.receive_scene(4096)
    lp.mode = mode
    return sd, rr.first_points(sd, lp, twin=class_ref.fluxmeter_twin(class_ref.receive_scene))


@pytest.mark.parametrize("mode", [capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ], ids=["raw", "iq"])
def test_populations_receive_through_the_twin(mode):
    sd, (d, p, shape) = _receive_points(mode)
    assert d.shape == p.shape == (4096, 3) and d.dtype == p.dtype == f32 and shape.shape == (4096,)
    assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-5)
    hit = shape >= 0
    assert set(np.unique(shape[hit])) == {2, 3} and not p[~hit].any()      # the ground and the bus; no path meets an aperture first
    # the point lies on the ray: p = o + t d to fp32 accuracy, o the aperture at (0, 0, 0.3) (20 x 50 mm)
    along = np.cross(p[hit].astype(np.float64) - (0.0, 0.0, 0.3), d[hit].astype(np.float64))
    assert np.abs(along).max() < 0.06
    for name in ("narrow", "wide", "half"):
        b = table(name)
        inside, outside, miss = _population(capi.range_rate_classes(d, p, shape, b, twists(sd)), b)
        assert inside.min() >= 1 and miss == int((~hit).sum()) > 0 and inside.sum() + outside + miss == 4096, (name, inside, outside, miss)
        assert (inside.tolist(), outside, miss) == POPULATIONS[("receive", name)], (name, inside, outside, miss)
    assert POPULATIONS[("receive", "narrow")][1] > 0          # the narrow table's class outside is populated
    # still twists: what a still scene returns to a moving radar is the ground's share of the window alone
    b = table("wide")
    at_rest = capi.range_rate_classes(d, p, shape, b, rr.still(sd))
    assert np.all(at_rest[hit] >= 8) and np.all(at_rest[hit] <= 15)      # rr = -4 d.x, 0 < d.x <= 1


def test_populations_film():
    sd, lp = class_ref.film_scene()
    b = table("film")
    d, p, shape = rr.first_points(sd, lp)
    inside, outside, miss = _population(capi.range_rate_classes(d, p, shape, b, twists(sd)), b)
    assert inside.min() >= 1 and outside > 0 and miss > 0 and inside.sum() + outside + miss == int(lp.n_paths), (inside, outside, miss)
    assert (inside.tolist(), outside, miss) == POPULATIONS[("film", "film")]


def test_populations_global_histogram_scene():
    sd, lp = scenes.bus_radar(n_tris=2000, n_paths=4096, bins=2560, dr=0.01, seed=7)
    b = table("global")
    d, p, shape = rr.first_points(sd, lp)
    inside, outside, miss = _population(capi.range_rate_classes(d, p, shape, b, twists(sd)), b)
    assert inside.min() >= 1 and outside > 0 and miss > 0 and inside.sum() + outside + miss == 4096, (inside, outside, miss)
    assert (inside.tolist(), outside, miss) == POPULATIONS[("global", "global")]


def test_library_exports_the_range_rate_entry():
    lib = C.CDLL(capi.LIB_PATH)
    assert "bf_scene_set_range_rate_classes" in capi.EXPORTED_SYMBOLS
    getattr(lib, "bf_scene_set_range_rate_classes")          # AttributeError: not exported
    text = open(HEADER).read()
    assert re.search(r"#define BF_ABI_VERSION 5\b", text) and capi.BF_ABI_VERSION == 5      # no struct or signature changed
    assert re.search(r"bf_scene_set_range_rate_classes\(bf_scene \*scene, const bf_range_rate_bins \*bins,\s+const bf_twist \*twists", text)
    assert C.sizeof(capi.bf_twist) == 36 and C.sizeof(capi.bf_range_rate_bins) == 24
    lib = capi.load_library()
    b = table("narrow")
    assert lib.bf_scene_set_range_rate_classes(None, C.byref(b), None, None) == capi.BF_ERR_INVALID
    assert b"bf_scene_set_range_rate_classes" in (lib.bf_last_error() or b"")
