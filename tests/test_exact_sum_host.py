"""BF_FLAG_EXACT_SUM without a GPU: the specification capi.exact_sum against fractions.Fraction arithmetic, the engine's accumulator
(beifong_amd/csrc/bf_sum.h through bf_exact_sum_host, and compiled into a host-only program) against the specification bit for bit,
the refusals of both entries, the constants, and the host layer's exact_sum option.

The expected values of the first test are derived here, independently of the code under test: the exact sum as a Fraction, rounded
to fp32 by choosing, among the fp32 neighbours of its double approximation, the one nearest in exact rational distance, ties to the
even mantissa; the hand-written results of tests/exact_sum_sets.py: EXPECTED are asserted on top."""
import ctypes as C
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from beifong_amd import capi
from tests import exact_sum_sets as sets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "beifong_amd", "host")
HEADER = os.path.join(ROOT, "include", "beifong_hip.h")
OVERFLOW = Fraction(2) ** 128 - Fraction(2) ** 103      # magnitudes from here on round to infinity


def fraction_to_f32(q):
    """q (a Fraction) rounded to fp32, nearest-even, by exact rational comparison"""
    if q == 0:
        return np.float32(0.0)
    if abs(q) >= OVERFLOW:
        return np.float32(np.inf if q > 0 else -np.inf)
    c = np.float32(float(q))      # within one fp32 step of the answer (two roundings)
    if np.isinf(c):
        c = np.float32(np.finfo(np.float32).max if q > 0 else -np.finfo(np.float32).max)
    with np.errstate(over="ignore"):      # (the neighbour of FLT_MAX is infinity: dropped below)
        cand = {float(np.nextafter(c, np.float32(-np.inf))), float(c), float(np.nextafter(c, np.float32(np.inf)))}
    cand = [x for x in cand if np.isfinite(x)]
    best = min(cand, key=lambda x: (abs(Fraction(x) - q), int(np.float32(x).view(np.uint32)) & 1))
    return np.float32(best)


def fraction_sums(cell, value, n_cells):
    tot = [Fraction(0)] * n_cells
    # (grouped by exponent first: Fractions of one exponent add as integers, which keeps 2^22 addends quick)
    v64 = value.astype(np.float64)
    m, e = np.frexp(v64)
    mant = np.round(np.ldexp(m, 24)).astype(np.int64)      # |m| < 1: a 24-bit integer, exact
    key, inv = np.unique(cell.astype(np.int64) * 4096 + (e.astype(np.int64) + 2048), return_inverse=True)
    part = np.zeros(key.size, np.int64)
    np.add.at(part, inv.reshape(-1), mant)
    for k, s in zip(key.tolist(), part.tolist()):
        tot[k // 4096] += Fraction(s) * Fraction(2) ** ((k % 4096) - 2048 - 24)
    return np.array([fraction_to_f32(q) for q in tot], np.float32)


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


ALL_SETS = sets.sets()


@pytest.mark.parametrize("name,cell,value,n_cells", ALL_SETS, ids=[s[0] for s in ALL_SETS])
def test_specification_against_fractions(name, cell, value, n_cells):
    want = fraction_sums(cell, value, n_cells)
    got = capi.exact_sum(cell, value, n_cells)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want)), (name, got, want)
    if name in sets.EXPECTED:
        hand = np.float32(sets.EXPECTED[name][1])
        assert bits(got)[0] == bits(hand), (name, got, hand)


def test_specification_by_hand_extremes():
    """what the sets' names promise, spelled out"""
    one = lambda vals: capi.exact_sum(np.zeros(len(vals), np.uint32), np.asarray(vals, np.float32), 1)[0]
    assert one([2.0 ** 24, 1.0]) == 2.0 ** 24 and one([2.0 ** 24 + 2, 1.0]) == 2.0 ** 24 + 4
    assert one([sets.FLT_MAX, 2.0 ** 102]) == np.float32(sets.FLT_MAX) and np.isposinf(one([sets.FLT_MAX, 2.0 ** 103]))
    assert np.isneginf(one([-sets.FLT_MAX, -2.0 ** 103]))
    assert bits(one([1.0, -1.0])) == 0 and bits(one([-0.0, -0.0])) == 0      # an exact zero is +0.0
    got = capi.exact_sum(np.asarray([2], np.uint32), np.asarray([1.5], np.float32), 4)
    assert got.tolist() == [0.0, 0.0, 1.5, 0.0] and not bits(got)[[0, 1, 3]].any()      # cells without addends
    straddle = dict((s[0], s) for s in ALL_SETS)
    assert np.isposinf(capi.exact_sum(*straddle["straddle_positive"][1:])[0])
    assert capi.exact_sum(*straddle["straddle_one_cell"][1:])[0] == 0.0
    alt = capi.exact_sum(*straddle["straddle_alternating"][1:])
    assert np.isposinf(alt[0]) and np.isneginf(alt[1])
    assert capi.exact_sum(*straddle["headroom"][1:])[0] == 0.0


@pytest.mark.parametrize("sign", [1, -1], ids=["positive", "negative"])
def test_specification_random_bit_patterns(sign):
    rng = np.random.default_rng(20 + sign)
    value = sets.random_bits(rng, 10000, sign)
    cell = rng.integers(0, 7, size=value.size).astype(np.uint32)
    want = fraction_sums(cell, value, 7)
    assert np.array_equal(bits(capi.exact_sum(cell, value, 7)), bits(want))
    # the same patterns over few exponents, so that the low bits decide: small magnitudes into one cell each, both signs
    small = (sets.random_bits(rng, 10000, None).view(np.uint32) & np.uint32(0x807fffff) | np.uint32(100 << 23))
    small = (small + (rng.integers(0, 40, size=small.size).astype(np.uint32) << np.uint32(23))).view(np.float32)
    want = fraction_sums(cell, small, 7)
    assert np.array_equal(bits(capi.exact_sum(cell, small, 7)), bits(want))


def _random_cases():
    rng = np.random.default_rng(5)
    out = []
    for sign in (1, -1, None):
        v = sets.random_bits(rng, 10000, sign)
        out.append((f"random_{sign}", rng.integers(0, 5, size=v.size).astype(np.uint32), v, 5))
    return out


HOST_CASES = ALL_SETS + _random_cases()


@pytest.mark.parametrize("name,cell,value,n_cells", HOST_CASES, ids=[s[0] for s in HOST_CASES])
def test_host_entry_equals_the_specification(hiplib, name, cell, value, n_cells):
    want = capi.exact_sum(cell, value, n_cells)
    for order, c, v in sets.orders(cell, value):
        got = capi.exact_sum_host(c, v, n_cells, hiplib)
        assert np.array_equal(bits(got), bits(want)), (name, order, got, want)


def test_accumulator_header_is_plain_cxx(tmp_path):
    """bf_sum.h compiles without HIP into a host-only program (tests/native/sum_check.cpp) and gives the specification's bits"""
    exe = tmp_path / "sum_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe), os.path.join(ROOT, "tests", "native", "sum_check.cpp")],
                   check=True)
    lines, want = [], []
    for name, cell, value, n_cells in ALL_SETS[:-1] + _random_cases()[-1:]:      # (all but the 2^22-addend set: text input)
        lines.append(f"{n_cells} {value.size}")
        lines += [f"{c} {b}" for c, b in zip(cell.tolist(), value.view(np.uint32).tolist())]
        want += bits(capi.exact_sum(cell, value, n_cells)).tolist()
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    assert [int(x) for x in out.split()] == want


def test_refusals_of_both_entries(hiplib):
    cell = np.asarray([0, 1], np.uint32)
    value = np.asarray([1.0, 2.0], np.float32)
    out = np.zeros(2, np.float32)
    p = capi._ptr
    for fn in (lambda *a: hiplib.bf_exact_sum_host(*a), lambda n, c, v, k, o: hiplib.bf_exact_sum(n, c, v, k, 0, o)):
        assert fn(2, None, p(value), 2, p(out)) == capi.BF_ERR_INVALID and b"null" in hiplib.bf_last_error()
        assert fn(2, p(cell), None, 2, p(out)) == capi.BF_ERR_INVALID
        assert fn(2, p(cell), p(value), 2, None) == capi.BF_ERR_INVALID
        assert fn(2, p(cell), p(value), 1, p(out)) == capi.BF_ERR_INVALID and b"cell[1] = 1 is not below n_cells 1" in hiplib.bf_last_error()
        for bad in (np.inf, -np.inf, np.nan):
            v = np.asarray([1.0, bad], np.float32)
            assert fn(2, p(cell), p(v), 2, p(out)) == capi.BF_ERR_INVALID and b"value[1] is not finite" in hiplib.bf_last_error()
        # the headroom is refused before an array is looked at
        assert fn(1 << 31, p(cell), p(value), 2, p(out)) == capi.BF_ERR_INVALID and b"2^31" in hiplib.bf_last_error()
    with pytest.raises(ValueError):
        capi.exact_sum(cell, value, 1)
    with pytest.raises(ValueError):
        capi.exact_sum(cell, np.asarray([1.0, np.inf], np.float32), 2)
    with pytest.raises(ValueError):
        capi.exact_sum(cell.astype(np.int64), value, 2)
    assert capi.exact_sum_host(cell[:0], value[:0], 3, hiplib).tolist() == [0.0, 0.0, 0.0]


def test_constants_and_symbols(hiplib):
    text = open(HEADER).read()
    assert re.search(r"\bBF_FLAG_EXACT_SUM = 4096u", text) and capi.BF_FLAG_EXACT_SUM == 4096
    assert re.search(r"\bBF_VARIANT_EXACT_SUM = 64\b", text) and capi.BF_VARIANT_EXACT_SUM == 64
    assert re.search(r"#define BF_ABI_VERSION 5\b", text) and hiplib.bf_version() == 5
    for sym in ("bf_exact_sum_host", "bf_exact_sum"):
        assert hasattr(hiplib, sym) and re.search(rf"\b{sym}\(", text) and sym in capi.EXPORTED_SYMBOLS
    for sym in ("bfk_launch_render_sum", "bfk_wf_shade_sum", "bfk_launch_tail_sum", "bfk_sum_resolve", "bfk_sum_probe"):
        assert hasattr(hiplib, sym), sym
    # the variant word: bf_variant.h restates bf_device.h
    dev = open(os.path.join(ROOT, "beifong_amd", "csrc", "bf_device.h")).read()
    var = open(os.path.join(ROOT, "beifong_amd", "csrc", "bf_variant.h")).read()
    assert re.search(r"\bkSum = 512\b", dev) and re.search(r"\bkSum = 512\b", var)
    assert re.search(r"enum Feature \{[^}]*kFeatSum = 4 \}", var)


@pytest.fixture(scope="module")
def mitsuba():
    if not os.path.exists(os.path.join(HOST, "libbeifong_host.so")):
        import __graft_entry__ as g
        g.build()
    from beifong_amd import mitsuba as m
    m.set_variant("scalar_rgb")
    return m


ON = '<boolean name="exact_sum" value="true"/>'


def test_host_layer_sets_the_flag(mitsuba):
    from beifong_amd.mitsuba.core.xml import load_dict, load_string
    from tests.test_host import RECEIVE_SCENE, TRANS_RAD_LIKE
    scene = load_string(TRANS_RAD_LIKE)
    assert not scene.integrator().launch_for(scene.sensors()[0]).flags & capi.BF_FLAG_EXACT_SUM
    # on the integrator that renders, and on a wrapper around it
    for xml in (TRANS_RAD_LIKE.replace('<integrator type="pathtime"/>', f'<integrator type="pathtime">{ON}</integrator>'),
                TRANS_RAD_LIKE.replace('<integrator type="time">', f'<integrator type="time">{ON}')):
        assert xml != TRANS_RAD_LIKE
        scene = load_string(xml)
        assert scene.integrator().launch_for(scene.sensors()[0]).flags & capi.BF_FLAG_EXACT_SUM
    scene = load_string(RECEIVE_SCENE.replace('<integrator type="pathtimefrequency"/>', f'<integrator type="pathtimefrequency">{ON}</integrator>'))
    assert scene.integrator().launch_for(scene.receivers()[0]).flags == capi.BF_FLAG_EXACT_SUM
    scene = load_string(RECEIVE_SCENE.replace('<integrator type="pathtimefrequency"/>',
                                              f'<integrator type="phase"><integer name="bins" value="4"/><integrator type="pathtimefrequency">{ON}</integrator></integrator>'))
    assert scene.integrator().launch_for(scene.receivers()[0]).flags == capi.BF_FLAG_EXACT_SUM
    for on in (False, True):
        sen = {"type": "perspective", "fov": 45, "sampler": {"type": "independent", "sample_count": 64},
               "film": {"type": "hdrfilm", "width": 1, "height": 1, "rfilter": {"type": "box"}}}
        scene = load_dict({"type": "scene", "sensor": sen,
                           "integrator": {"type": "range", "dr": 0.2, "bins": 8, "exact_sum": on, "integrator": {"type": "pathlength"}}})
        assert bool(scene.integrator().launch_for(scene.sensors()[0]).flags & capi.BF_FLAG_EXACT_SUM) == on


def test_host_layer_refuses_by_name(mitsuba):
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_aov_host import PATH, _xml
    from tests.test_host import TRANS_RAD_LIKE
    from tests.test_moment_host import MOMENT_XML
    fast = '<boolean name="fast_math" value="true"/>'
    # fast_math: on the same integrator, above and below
    for xml in (TRANS_RAD_LIKE.replace('<integrator type="pathtime"/>', f'<integrator type="pathtime">{ON}{fast}</integrator>'),
                TRANS_RAD_LIKE.replace('<integrator type="time">', f'<integrator type="time">{fast}').replace(
                    '<integrator type="pathtime"/>', f'<integrator type="pathtime">{ON}</integrator>'),
                TRANS_RAD_LIKE.replace('<integrator type="time">', f'<integrator type="time">{ON}').replace(
                    '<integrator type="pathtime"/>', f'<integrator type="pathtime">{fast}</integrator>')):
        with pytest.raises(_host.HostError, match='"exact_sum" with "fast_math"'):
            load_string(xml)
    # a moment integrator above (the option below it, at either depth) or carrying the option itself
    for xml in (MOMENT_XML.replace('<integrator type="moment">', f'<integrator type="moment">{ON}'),
                MOMENT_XML.replace('<integrator type="range" name="nested">', f'<integrator type="range" name="nested">{ON}'),
                MOMENT_XML.replace('<integrator type="pathlength">', f'<integrator type="pathlength">{ON}')):
        assert xml != MOMENT_XML
        with pytest.raises(_host.HostError, match='"exact_sum" with a "moment" integrator'):
            load_string(xml)
    # an aov integrator, likewise
    for xml in (_xml(PATH).replace('<integrator type="aov">', f'<integrator type="aov">{ON}'),
                _xml(PATH.replace("/>", f">{ON}</integrator>"))):
        with pytest.raises(_host.HostError, match='"exact_sum" with an "aov" integrator'):
            load_string(xml)
    # more than one GPU
    mitsuba.set_gpu_count(2)
    try:
        with pytest.raises(_host.HostError, match='"exact_sum" renders on one GPU.*gpu_count is 2'):
            load_string(TRANS_RAD_LIKE.replace('<integrator type="time">', f'<integrator type="time">{ON}'))
    finally:
        mitsuba.set_gpu_count(1)
    # ... also when the count changes after construction: refused when the launch is made
    scene = load_string(TRANS_RAD_LIKE.replace('<integrator type="time">', f'<integrator type="time">{ON}'))
    mitsuba.set_gpu_count(2)
    try:
        with pytest.raises(_host.HostError, match='"exact_sum" renders on one GPU'):
            scene.integrator().launch_for(scene.sensors()[0])
    finally:
        mitsuba.set_gpu_count(1)
