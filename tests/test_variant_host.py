"""Which bf_render_kernel instantiation a launch runs (beifong_amd/csrc/bf_variant.h: render_variant, tail_variant), walked on the
CPU through a host-only program (tests/native/variant_check.cpp) over every combination of kind (render, tail), feature (none,
moment, class, aov, sum) and launch shape (geom_stride, wide, lean, multi, tail_waves == 2, roll, mode == RECEIVE_RAW), and held against
the if-chains render_launch and tail_launch consisted of before the selector existed, restated here by hand, chain by chain.

The same for wf_shade's <FIRST, W, V> (shade_variant: feature x fast / exact object x first 0-3 x requested waves 0-5 x shape) and
wf_trace's <STATS, W, SHIFT, QUANT, GEOM> (trace_variant: stats x waves 3-7 x shift x quant x geom), against the macro chains of
wf_shade_launch and bfk_wf_trace they replaced; and the selectors' ranges against the sets of instantiations bf_variant.h states for
the launchers to instantiate (shade_exists, trace_exists)."""
import itertools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the variant word of bf_device.h
WIDE, LEAN, MULTI, GEOM, MOMENT, CLASS, AOV, SUM = 4, 8, 16, 32, 64, 128, 256, 512
TAIL_TWO = 1 << 16      # bf_variant.h: the general tail kernel at two waves per SIMD, <S, true, P, 2>
INVALID = -1
PLAIN, F_MOMENT, F_CLASS, F_AOV, F_SUM = 0, 1, 2, 3, 4
FEATURES = (PLAIN, F_MOMENT, F_CLASS, F_AOV, F_SUM)
REFUSED = (-1, 0, 0)      # bf_variant.h: kRefused


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
    if feature == F_SUM:
        if multi or roll:
            return INVALID
        return SUM | _four_forms(geom, wide)
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
    if feature == F_SUM:
        if multi or roll:
            return INVALID
        return SUM | _four_forms(geom, wide)
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


# ---- wf_shade_launch, chain by chain: (FIRST, W, V), V = mode class | variant bits ----
def _first_of_four(first):
    """if (first == 3) <3>; else if (first == 2) <2>; else if (first) <1>; else <0>"""
    if first == 3:
        return 3
    if first == 2:
        return 2
    return 1 if first else 0


def _geom_form(wide, lean):
    """if (lean && !wide) kGeom | kLean; else if (wide) kGeom | kWide; else kGeom"""
    if lean and not wide:
        return GEOM | LEAN
    if wide:
        return GEOM | WIDE
    return GEOM


def _shade_moment(first, geom, wide, lean, multi, raw):
    rx = 1 if raw else 0
    if geom:
        if first >= 2:
            return REFUSED
        return (1 if first else 0, 3, rx | MOMENT | _geom_form(wide, lean))
    if multi:
        return (_first_of_four(first), 3, rx | MOMENT | MULTI)
    if lean and not wide:
        return (_first_of_four(first), 3, rx | MOMENT | LEAN)
    if wide:
        return (_first_of_four(first), 3, rx | MOMENT | WIDE)
    return (_first_of_four(first), 3, rx | MOMENT)


def _shade_class(first, geom, wide, multi, roll, raw):
    if first >= 2 or multi or roll:
        return REFUSED
    return (1 if first else 0, 3, (1 if raw else 0) | CLASS | _four_forms(geom, wide))


def _shade_aov(first, geom, wide, roll, raw):
    if first >= 2 or raw or roll:
        return REFUSED
    return (1 if first else 0, 3, 0 | AOV | _four_forms(geom, wide))


def _shade_sum(first, geom, wide, multi, roll, raw):
    if first >= 2 or multi or roll:
        return REFUSED
    return (1 if first else 0, 3, (1 if raw else 0) | SUM | _four_forms(geom, wide))


def _shade_plain(first, waves, geom, wide, lean, multi, raw):
    rx = 1 if raw else 0
    # gen4 = waves == 4 && bfk_shade_gen4(*lp, first), where bfk_shade_gen4 was:
    #   if (!lean || wide || multi || geom_stride) false; else first == 1 || (first == 2 && mode != RECEIVE_RAW)
    gen4 = waves == 4 and not (not lean or wide or multi or geom) and (first == 1 or (first == 2 and not raw))
    if geom:
        if first >= 2:
            return REFUSED
        return (1 if first else 0, 3, rx | _geom_form(wide, lean))
    if multi:
        return (_first_of_four(first), 3, rx | MULTI)
    if lean and not wide and (first or waves == 3):
        if first == 3:
            return (3, 3, rx | LEAN)
        if first == 2 and gen4:
            return (2, 4, 0 | LEAN)
        if first == 2:
            return (2, 3, rx | LEAN)
        if first and gen4:
            return (1, 4, rx | LEAN)
        if first:
            return (1, 3, rx | LEAN)
        return (0, 3, rx | LEAN)
    if wide:
        return (_first_of_four(first), 3, rx | WIDE)
    if first == 3:
        return (3, 3, rx)
    if first == 2:
        return (2, 3, rx)
    if first:
        return (1, 3, rx)
    return (0, waves if waves in (2, 3, 4) else 1, rx)


def expected_shade(feature, fast, first, waves, geom, wide, lean, multi, two, roll, raw):
    if fast and feature != PLAIN:      # #if BF_FAST: if (moment || classed || aov || sum) return hipErrorInvalidValue
        return REFUSED
    if feature == F_MOMENT:
        return _shade_moment(first, geom, wide, lean, multi, raw)
    if feature == F_CLASS:
        return _shade_class(first, geom, wide, multi, roll, raw)
    if feature == F_AOV:
        return _shade_aov(first, geom, wide, roll, raw)
    if feature == F_SUM:
        return _shade_sum(first, geom, wide, multi, roll, raw)
    return _shade_plain(first, waves, geom, wide, lean, multi, raw)


def expected_trace(stats, waves, shift, quant, geom):
    """bfk_wf_trace: (STATS, W, SHIFT, QUANT, GEOM)"""
    if geom:      # wf_trace<S, W, false, quant, true>, W = 5 if waves >= 5 else 4: `shift` is not looked at
        return (stats, 5 if waves >= 5 else 4, 0, quant, 1)
    if waves >= 6 and quant:
        return (stats, 6, shift, 1, 0)
    if waves >= 5:
        return (stats, 5, shift, quant, 0)
    return (stats, 4, shift, quant, 0)


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    """the lines of variant_check by their leading kind: {kind: {inputs: outputs}}"""
    exe = tmp_path_factory.mktemp("variant") / "variant_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-o", str(exe),
                    os.path.join(ROOT, "tests", "native", "variant_check.cpp")], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    n_in = {0: 8, 1: 8, 2: 11, 3: 5, 4: 4, 5: 5}
    rows = {k: {} for k in n_in}
    for line in out.splitlines():
        v = [int(x) for x in line.split()]
        key, val = tuple(v[1:1 + n_in[v[0]]]), tuple(v[1 + n_in[v[0]]:])
        assert key not in rows[v[0]]
        rows[v[0]][key] = val
    return rows


@pytest.fixture(scope="module")
def table(walk):
    """render_variant and tail_variant: (kind, feature, shape...) -> word"""
    return {(kind,) + key: val[0] for kind in (0, 1) for key, val in walk[kind].items()}


def test_every_combination_is_walked(table, walk):
    assert len(table) == 2 * 5 * 2 ** 7
    assert len(walk[2]) == 5 * 2 * 4 * 6 * 2 ** 7 and len(walk[3]) == 2 * 5 * 2 ** 3


@pytest.mark.parametrize("kind", [0, 1], ids=["render", "tail"])
def test_selector_matches_the_former_if_chains(table, kind):
    want = expected_tail if kind else expected_render
    bad = []
    for feature in FEATURES:
        for shape in itertools.product((0, 1), repeat=7):      # geom wide lean multi two roll raw
            got = table[(kind, feature) + shape]
            if got != want(feature, *shape):
                bad.append((feature, shape, got, want(feature, *shape)))
    assert not bad, bad[:8]


def test_the_words_are_the_instantiations_that_exist(table):
    """20 render forms (the four general forms of the five families) and 27 tail forms (the plain family's eight, the moment family's
    seven, the four general forms of the class, AOV and exact-sum families), times STATS and SPILL: 4 x (20 + 27) = 188, the number of
    bf_render_kernel instantiations `make resource-usage` lists for the exact bf_kernels.hip (profiles/variant_resource_usage.txt)."""
    render = {w for k, w in table.items() if k[0] == 0 and w != INVALID}
    tail = {w for k, w in table.items() if k[0] == 1 and w != INVALID}
    forms = {0, WIDE, GEOM, WIDE | GEOM}
    assert render == {f | v for f in (0, MOMENT, CLASS, AOV, SUM) for v in forms}
    tail_plain = forms | {LEAN, LEAN | GEOM, MULTI}
    assert tail == tail_plain | {TAIL_TWO} | {MOMENT | v for v in tail_plain} | {f | v for f in (CLASS, AOV, SUM) for v in forms}
    assert 4 * (len(render) + len(tail)) == 188


def test_shade_selector_matches_the_former_macro_chains(walk):
    bad = []
    for key in itertools.product(FEATURES, (0, 1), range(4), range(6), *[(0, 1)] * 7):      # feature fast first waves + the shape
        got, want = walk[2][key], expected_shade(*key)
        if got != want:
            bad.append((key, got, want))
    assert not bad, bad[:8]


def test_trace_selector_matches_the_former_macro_chains(walk):
    bad = []
    for key in itertools.product((0, 1), range(3, 8), (0, 1), (0, 1), (0, 1)):      # stats waves shift quant geom
        got, want = walk[3][key], expected_trace(*key)
        if got != want:
            bad.append((key, got, want))
    assert not bad, bad[:8]


def test_shade_forms_are_the_instantiations_that_exist(walk):
    """What the selector can answer is what bf_variant.h states the object holds (shade_exists), the fast and the exact object apart.
    The fast object, 53 = the plain family: per-render geometry 2 firsts x 3 forms x 2 mode classes = 12; per-path tables 4 x 2 = 8;
    lean 4 x 2 at three waves + <1, 4> of both mode classes + <2, 4> of the render modes = 11; wide 4 x 2 = 8; general 3 x 2 at three
    waves + the walk at 1, 2, 3, 4 x 2 = 14.  The exact object, 137 = those 53 + the moment family's 12 + (multi, lean, wide, general) x 4
    firsts x 2 = 44 + class and exact sum 2 firsts x 4 forms x 2 each = 32 + AOV 2 x 4 = 8.  `make resource-usage` /
    `resource-usage-fast` list as many wf_shade kernels (profiles/variant_resource_usage.txt)."""
    for fast, n in ((0, 137), (1, 53)):
        stated = {k[1:] for k in walk[4] if k[0] == fast}
        reached = {v for k, v in walk[2].items() if k[1] == fast and v != REFUSED}
        assert reached == stated and len(stated) == n, (fast, sorted(reached ^ stated)[:8], len(stated))


def test_trace_forms_are_the_instantiations_that_exist(walk):
    """28 per object = STATS x (W 4, 5 x SHIFT x QUANT = 8, W 6 quantised x SHIFT = 2, per-render geometry W 4, 5 x QUANT = 4)"""
    stated, reached = set(walk[5]), set(walk[3].values())
    assert reached == stated and len(stated) == 28, sorted(reached ^ stated)[:8]
