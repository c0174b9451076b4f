"""Which bf_render_kernel instantiation a launch runs (beifong_amd/csrc/bf_variant.h: render_variant, tail_variant), walked on the
CPU through a host-only program (tests/native/variant_check.cpp) over every combination of kind (render, tail), feature (none,
moment, class, aov) and launch shape (geom_stride, wide, lean, multi, tail_waves == 2, roll, mode == RECEIVE_RAW), and held against
the if-chains render_launch and tail_launch consisted of before the selector existed, restated here by hand, chain by chain."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the variant word of bf_device.h
WIDE, LEAN, MULTI, GEOM, MOMENT, CLASS, AOV = 4, 8, 16, 32, 64, 128, 256
TAIL_TWO = 1 << 16      # bf_variant.h: the general tail kernel at two waves per SIMD, <S, true, P, 2>
INVALID = -1
PLAIN, F_MOMENT, F_CLASS, F_AOV = 0, 1, 2, 3


def _four_forms(geom, wide):
    """if (geom_stride && wide) kWide | kGeom; else if (geom_stride) kGeom; else if (wide) kWide; else 0"""
    if geom and wide:
        return WIDE | GEOM
    if geom:
        return GEOM
    if wide:
        return WIDE
    return 0


def expected_render(feature, geom, wide, lean, multi, two, roll, raw):
    if feature == F_MOMENT:
        return MOMENT | _four_forms(geom, wide)
    if feature == F_CLASS:
        return CLASS | _four_forms(geom, wide)
    if feature == F_AOV:
        if raw or roll:
            return INVALID
        return AOV | _four_forms(geom, wide)
    if geom:
        return (WIDE | GEOM) if wide else GEOM
    return WIDE if wide else 0


def expected_tail(feature, geom, wide, lean, multi, two, roll, raw):
    if feature == F_MOMENT:      # always three waves per SIMD
        if geom and wide:
            return MOMENT | WIDE | GEOM
        if geom and lean:
            return MOMENT | LEAN | GEOM
        if geom:
            return MOMENT | GEOM
        if multi:
            return MOMENT | MULTI
        if wide:
            return MOMENT | WIDE
        if lean:
            return MOMENT | LEAN
        return MOMENT
    if feature == F_CLASS:
        if multi or roll:
            return INVALID
        return CLASS | _four_forms(geom, wide)
    if feature == F_AOV:
        if raw or roll:
            return INVALID
        return AOV | _four_forms(geom, wide)
    if geom and wide:
        return WIDE | GEOM
    if geom and lean:
        return LEAN | GEOM
    if geom:
        return GEOM
    if multi:
        return MULTI
    if wide:
        return WIDE
    if lean and not two:
        return LEAN
    if two:
        return TAIL_TWO
    return 0


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = tmp_path_factory.mktemp("variant") / "variant_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "variant_check.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    rows = {}
    for line in out.splitlines():
        v = [int(x) for x in line.split()]
        assert tuple(v[:9]) not in rows
        rows[tuple(v[:9])] = v[9]
    return rows


def test_every_combination_is_walked(table):
    assert len(table) == 2 * 4 * 2 ** 7


@pytest.mark.parametrize("kind", [0, 1], ids=["render", "tail"])
def test_selector_matches_the_former_if_chains(table, kind):
    want = expected_tail if kind else expected_render
    bad = []
    for feature in (PLAIN, F_MOMENT, F_CLASS, F_AOV):
        for shape in itertools.product((0, 1), repeat=7):      # geom wide lean multi two roll raw
            got = table[(kind, feature) + shape]
            if got != want(feature, *shape):
                bad.append((feature, shape, got, want(feature, *shape)))
    assert not bad, bad[:8]


def test_the_words_are_the_instantiations_that_exist(table):
    """16 render forms and 23 tail forms (times STATS and SPILL: the 156 bf_render_kernel instantiations of the exact build)."""
    render = {w for k, w in table.items() if k[0] == 0 and w != INVALID}
    tail = {w for k, w in table.items() if k[0] == 1 and w != INVALID}
    forms = {0, WIDE, GEOM, WIDE | GEOM}
    assert render == {f | v for f in (0, MOMENT, CLASS, AOV) for v in forms}
    tail_plain = forms | {LEAN, LEAN | GEOM, MULTI}
    assert tail == tail_plain | {TAIL_TWO} | {MOMENT | v for v in tail_plain} | {f | v for f in (CLASS, AOV) for v in forms}
    assert 4 * (len(render) + len(tail)) == 156
