"""BF_FLAG_MOMENT without a GPU: channel counts of the C ABI, the `moment` plugin, the Python helpers, and the agreement of
the two ways tests/moment_ref.py derives expected second moments from the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

from beifong_amd import capi, scenes
from tests import moment_ref as mr
from tests.oracle_lib import OracleScene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "beifong_amd", "host")


@pytest.fixture(scope="module")
def mitsuba():
    if not os.path.exists(os.path.join(HOST, "plugins", "moment.so")):
        import __graft_entry__ as g
        g.build()
    from beifong_amd import mitsuba as m
    m.set_variant("scalar_rgb")
    return m


def _channels(lib, **kw):
    lp = capi.make_launch(**kw)
    lib.bf_launch_channels.restype = C.c_uint32
    return lib.bf_launch_channels(C.byref(lp))


def test_launch_channels_with_the_flag(hiplib):
    F = capi.BF_FLAG_MOMENT
    assert F == 512 and capi.BF_VARIANT_MOMENT == 8
    assert hiplib.bf_version() == 5
    bins = 7
    for film, px in ((None, 1), ((5, 3), 15)):
        kw = dict(n_paths=px * 4, film=film, spp=4 if film else 0)
        assert _channels(hiplib, mode=capi.BF_MODE_PATH, flags=F, **kw) == px * 11                   # 5 + 2 (0 + 3)
        assert _channels(hiplib, mode=capi.BF_MODE_RANGE, bins=bins, bin_width=1.0, flags=F, **kw) == px * (5 + 2 * (bins + 3))
        assert _channels(hiplib, mode=capi.BF_MODE_TIME, bins=bins, bin_width=1.0, flags=F, **kw) == px * (5 + 2 * (3 * bins + 3))
        # without the flag nothing moved
        assert _channels(hiplib, mode=capi.BF_MODE_RANGE, bins=bins, bin_width=1.0, **kw) == px * (5 + bins)
    assert _channels(hiplib, mode=capi.BF_MODE_RECEIVE_RAW, n_paths=4, bins=8, bins_y=4, flags=F) == 32 * 4
    assert _channels(hiplib, mode=capi.BF_MODE_RECEIVE_RAW, n_paths=4, bins=8, bins_y=4, phase_bins=4, flags=F) == 32 * 8
    assert _channels(hiplib, mode=capi.BF_MODE_RECEIVE_IQ, n_paths=4, bins=8, bins_y=4, flags=F) == 32 * 5
    assert _channels(hiplib, mode=capi.BF_MODE_RECEIVE_IQ, n_paths=4, bins=8, bins_y=4) == 32 * 3


def test_moment_layout_pairs_every_first_moment_channel():
    lp = capi.make_launch(capi.BF_MODE_RANGE, 8, bins=4, bin_width=1.0, flags=capi.BF_FLAG_MOMENT)
    first, second = capi.moment_layout(lp)
    # X Y Z A W | S0-S3 | n.X n.Y n.Z | m2_S0-S3 | m2_n.X .Y .Z
    assert first.tolist() == [[5, 6, 7, 8, 9, 10, 11]] and second.tolist() == [[12, 13, 14, 15, 16, 17, 18]]
    lp = capi.make_launch(capi.BF_MODE_TIME, 8, bins=2, bin_width=1.0, flags=capi.BF_FLAG_MOMENT, film=(2, 1), spp=4)
    first, second = capi.moment_layout(lp)
    assert first.shape == (2, 9) and first[1, 0] == 23 + 5 and second[1, -1] == 2 * 23 - 1 and second[0, 0] == 5 + 9
    lp = capi.make_launch(capi.BF_MODE_PATH, 8, flags=capi.BF_FLAG_MOMENT)
    assert [a.tolist() for a in capi.moment_layout(lp)] == [[[5, 6, 7]], [[8, 9, 10]]]
    lp = capi.make_launch(capi.BF_MODE_RECEIVE_RAW, 8, bins=2, bins_y=1, phase_bins=3, flags=capi.BF_FLAG_MOMENT)
    assert [a.tolist() for a in capi.moment_layout(lp)] == [[[0], [7]], [[6], [13]]]
    lp = capi.make_launch(capi.BF_MODE_RECEIVE_IQ, 8, bins=2, bins_y=1, flags=capi.BF_FLAG_MOMENT)
    assert [a.tolist() for a in capi.moment_layout(lp)] == [[[0, 1], [5, 6]], [[3, 4], [8, 9]]]
    with pytest.raises(ValueError):
        capi.moment_layout(capi.make_launch(capi.BF_MODE_PATH, 8))


def test_moment_estimate_closed_forms():
    n = 1000
    lp = capi.make_launch(capi.BF_MODE_PATH, n, flags=capi.BF_FLAG_MOMENT)
    # n identical samples 3: variance 0; nested.Y: samples {0, 2} in equal numbers; nested.Z: nothing
    h = np.zeros(11)
    h[4] = n
    h[5], h[8] = 3.0 * n, 9.0 * n
    h[6], h[9] = 2.0 * n / 2, 4.0 * n / 2
    mean, var, rel = capi.moment_estimate(h, lp)
    assert mean.shape == (1, 3) and mean.dtype == np.float64
    assert mean[0].tolist() == [3.0, 1.0, 0.0]
    assert var[0, 0] == 0.0 and rel[0, 0] == 0.0
    # E x^2 - mean^2 = 2 - 1 = 1, over n - 1
    assert np.isclose(var[0, 1], 1.0 / (n - 1), rtol=1e-15) and np.isclose(rel[0, 1], np.sqrt(1.0 / (n - 1)), rtol=1e-15)
    assert var[0, 2] == 0.0 and np.isinf(rel[0, 2])
    # ADC cells and pixels take n from their own W
    lp = capi.make_launch(capi.BF_MODE_RECEIVE_IQ, n, bins=2, bins_y=1, flags=capi.BF_FLAG_MOMENT)
    h = np.array([10.0, -10.0, 10.0, 10.0, 10.0, 0.0, 20.0, 40.0, 0.0, 20.0])
    mean, var, rel = capi.moment_estimate(h, lp)
    assert mean.tolist() == [[1.0, -1.0], [0.0, 0.5]] and var[0].tolist() == [0.0, 0.0]
    assert np.isinf(rel[1, 0]) and np.isclose(var[1, 1], (20.0 / 40 - 0.25) / 39)
    with pytest.raises(ValueError):
        capi.moment_estimate(h[:-1], lp)


MOMENT_XML = """
<scene version="2.1.0">
    <integrator type="moment">
        <integrator type="range" name="nested"><integrator type="pathlength"><integer name="max_depth" value="3"/></integrator>
            <float name="dr" value="0.5"/><integer name="bins" value="4"/></integrator>
    </integrator>
    <sensor type="perspective">
        <transform name="to_world"><lookat origin="0, 0, 0" target="0, -1, 0" up="0, 0, 1"/></transform>
        <film type="hdrfilm"><integer name="width" value="1"/><integer name="height" value="1"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="64"/></sampler>
    </sensor>
    <emitter type="spot"><spectrum value="10" name="intensity"/>
        <transform name="to_world"><lookat origin="0, 0, 0" target="0, -1, 0" up="0, 0, 1"/></transform></emitter>
    <shape type="rectangle"><transform name="to_world"><lookat origin="0, -1, 0" target="0, 0, 0" up="0, 0, 1"/></transform>
        <bsdf type="twosided"><bsdf type="diffuse"/></bsdf></shape>
</scene>
"""


def test_moment_plugin_names_and_launch(mitsuba):
    from beifong_amd.mitsuba.core.xml import load_string
    scene = load_string(MOMENT_XML)
    integ = scene.integrator()
    # moment.cpp:39-52 written out: <child>.<nested aov> ..., <child>.X .Y .Z, then m2_ of each
    assert integ.aov_names() == ["nested.S0.Y", "nested.S1.Y", "nested.S2.Y", "nested.S3.Y", "nested.X", "nested.Y", "nested.Z",
                                 "m2_nested.S0.Y", "m2_nested.S1.Y", "m2_nested.S2.Y", "m2_nested.S3.Y", "m2_nested.X", "m2_nested.Y",
                                 "m2_nested.Z"]
    lp = integ.launch_for(scene.sensors()[0])
    assert (lp.mode, lp.bins, lp.max_depth, lp.flags & capi.BF_FLAG_MOMENT, lp.n_paths) == (capi.BF_MODE_RANGE, 4, 3, 512, 64)
    assert capi.load_library().bf_launch_channels(C.byref(lp)) == 5 + len(integ.aov_names())
    # the flag changes nothing the oracle sees: the launch without it is the nested integrator's
    h = OracleScene(scene.flat_desc(scene.sensors()[0])).render(mr.plain(lp))[0]
    assert h.shape == (9,) and h[4] == 64


def test_moment_plugin_refusals(mitsuba):
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    two = MOMENT_XML.replace("</integrator>\n    </integrator>", "</integrator>\n        <integrator type=\"path\" name=\"second\"/>\n    </integrator>")
    assert two != MOMENT_XML
    with pytest.raises(_host.HostError, match="more than one nested integrator.*second"):
        load_string(two)
    for fast in (MOMENT_XML.replace('<integrator type="moment">', '<integrator type="moment"><boolean name="fast_math" value="true"/>'),
                 MOMENT_XML.replace('<integrator type="pathlength">', '<integrator type="pathlength"><boolean name="fast_math" value="true"/>')):
        assert fast != MOMENT_XML
        with pytest.raises(_host.HostError, match="fast_math"):
            load_string(fast)
    with pytest.raises(_host.HostError, match="sub-integrator"):
        load_string('<scene version="2.1.0"><integrator type="moment"/></scene>')


def test_moment_load_dict_matches_xml(mitsuba):
    from beifong_amd.mitsuba.core import Transform4f
    from beifong_amd.mitsuba.core.xml import load_dict, load_string
    look = Transform4f.look_at([0, 0, 0], [0, -1, 0], [0, 0, 1])
    scene = load_dict({
        "type": "scene",
        "integrator": {"type": "moment", "nested": {"type": "range", "integrator": {"type": "pathlength", "max_depth": 3}, "dr": 0.5, "bins": 4}},
        "sensor": {"type": "perspective", "to_world": look, "sampler": {"type": "independent", "sample_count": 64},
                   "film": {"type": "hdrfilm", "rfilter": {"type": "box"}, "width": 1, "height": 1}},
        "emitter": {"type": "spot", "intensity": {"type": "spectrum", "value": 10}, "to_world": look},
        "shape": {"type": "rectangle", "to_world": Transform4f.look_at([0, -1, 0], [0, 0, 0], [0, 0, 1]),
                  "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse"}}},
    })
    ref = load_string(MOMENT_XML)
    a, b = scene.integrator().launch_for(scene.sensors()[0]), ref.integrator().launch_for(ref.sensors()[0])
    assert bytes(a) == bytes(b)
    assert scene.integrator().aov_names() == ref.integrator().aov_names()


def test_moment_receive_names(mitsuba):
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_host import RECEIVE_SCENE
    xml = RECEIVE_SCENE.replace('<integrator type="pathtimefrequency"/>',
                                '<integrator type="moment"><integrator type="phase"><integer name="bins" value="3"/>'
                                '<integrator type="pathtimefrequency"/></integrator></integrator>')
    scene = load_string(xml)
    assert scene.integrator().aov_names() == ["S0.Y", "S1.Y", "S2.Y", "m2_Y"]
    lp = scene.integrator().launch_for(scene.receivers()[0])
    assert lp.mode == capi.BF_MODE_RECEIVE_RAW and lp.phase_bins == 3 and lp.flags & capi.BF_FLAG_MOMENT
    assert capi.load_library().bf_launch_channels(C.byref(lp)) == lp.bins * lp.bins_y * 7


def test_both_derivations_of_the_expected_moments_agree():
    """tests/moment_ref.py: per-path oracle renders against the records of one oracle render (weight 1, 1 x 1 film)"""
    for color in (capi.BF_COLOR_RGB, capi.BF_COLOR_MONO):
        sd, lp = scenes.bus_radar(n_tris=2000, n_paths=192, bins=16, dr=1.6, seed=3)
        lp.color_mode = color
        osc = OracleScene(sd)
        _, rec, _ = osc.render(lp, records=True)
        a = mr.from_records(rec, lp)
        ref, S, N, E2 = mr.single_paths(osc, lp)
        b = mr.m2_from_single(E2, N, lp, weight_one=True)
        assert b.sel.all() and np.array_equal(a.N, b.N) and a.N[:16].sum() > 20
        # the AOV cells hold L itself: the same squares, summed in the same order
        assert np.array_equal(a.E[:16], b.E[:16])
        # nested.XYZ: the float64 recomputation against the fp32 cell values (three roundings each way, squared)
        assert np.allclose(a.E[16:], b.E[16:], rtol=8 * 2.0 ** -24, atol=0.0)
        # and the single-path sums are the oracle's own addends
        _, _, _, add = osc.render(lp, addends=True)
        assert np.array_equal(N, add.N) and np.allclose(ref, add.ref, rtol=1e-12) and np.allclose(S, add.S, rtol=1e-12)
