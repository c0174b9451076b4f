"""BF_FLAG_AOV without a GPU: bf_aov_floats and the constants of the C ABI, the Python helpers, and the `aov` plugin — channel
names in the reference's order (aov.cpp:83-150), its error texts, its refusals, and load_dict against load_string."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from beifong_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "beifong_amd", "host")
HEADER = os.path.join(ROOT, "include", "beifong_hip.h")


@pytest.fixture(scope="module")
def mitsuba():
    if not os.path.exists(os.path.join(HOST, "plugins", "aov.so")):
        import __graft_entry__ as g
        g.build()
    from beifong_amd import mitsuba as m
    m.set_variant("scalar_rgb")
    return m


def test_aov_floats(hiplib):
    f = lambda t: capi.aov_floats(np.asarray(t, np.uint32), hiplib)
    assert [f([t]) for t in range(capi.BF_AOV_TYPES)] == [1, 3, 2, 3, 3, 3, 3, 2, 2] == list(capi.AOV_TYPE_FLOATS)
    assert f(list(range(capi.BF_AOV_TYPES))) == 22
    assert f([capi.BF_AOV_DEPTH, capi.BF_AOV_SH_NORMAL, capi.BF_AOV_DEPTH]) == 5          # a type may repeat
    assert f([capi.BF_AOV_POSITION] * capi.BF_MAX_AOVS) == 48
    # invalid lists: empty, too long, an unknown type, a null pointer
    assert f([]) == 0 and f([0] * (capi.BF_MAX_AOVS + 1)) == 0 and f([capi.BF_AOV_TYPES]) == 0 and f([0, 1000]) == 0
    assert hiplib.bf_aov_floats(3, None) == 0


def test_constants_match_the_header(hiplib):
    text = open(HEADER).read()
    assert re.search(r"BF_FLAG_AOV = 2048u", text) and capi.BF_FLAG_AOV == 2048
    assert re.search(r"BF_VARIANT_AOV = 32\b", text) and capi.BF_VARIANT_AOV == 32
    assert re.search(r"#define BF_MAX_AOVS 16\b", text) and capi.BF_MAX_AOVS == 16
    assert re.search(r"#define BF_ABI_VERSION 5\b", text) and hiplib.bf_version() == 5
    enum = re.search(r"enum \{ (BF_AOV_DEPTH = 0,.*?BF_AOV_TYPES) \};", text, re.S).group(1)
    names = re.findall(r"BF_AOV_[A-Z_]+", re.sub(r"/\*.*?\*/", "", enum, flags=re.S))
    assert names == ["BF_AOV_DEPTH", "BF_AOV_POSITION", "BF_AOV_UV", "BF_AOV_GEO_NORMAL", "BF_AOV_SH_NORMAL", "BF_AOV_DP_DU",
                     "BF_AOV_DP_DV", "BF_AOV_DUV_DX", "BF_AOV_DUV_DY", "BF_AOV_TYPES"]
    assert [getattr(capi, n) for n in names] == list(range(10))
    assert ["BF_AOV_" + n.upper() for n in capi.AOV_TYPE_NAMES] == names[:-1]
    for sym in ("bf_aov_floats", "bf_scene_set_aovs"):      # exported, and declared
        assert hasattr(hiplib, sym) and re.search(rf"\b{sym}\(", text)


def test_python_helpers():
    assert capi.aov_types(["depth", "sh_normal", 1]).tolist() == [0, 4, 1]
    with pytest.raises(ValueError, match="unknown AOV type 'normal'"):
        capi.aov_types(["normal"])
    lp = capi.make_launch(capi.BF_MODE_RANGE, 8, bins=4, bin_width=1.0, flags=capi.BF_FLAG_AOV)
    lay = capi.aov_layout(lp, ["depth", "uv", "depth", "sh_normal"])
    # X Y Z A W | d u v d nx ny nz | S0-S3 | R G B A
    assert lay["K"] == 7 and lay["chan_px"] == 5 + 7 + 4 + 4
    assert [(s.start, s.stop) for s in lay["aovs"]] == [(5, 6), (6, 8), (8, 9), (9, 12)]
    assert lay["names"] == {"depth": slice(5, 6), "uv": slice(6, 8), "sh_normal": slice(9, 12)}
    assert lay["nested"] == slice(12, 16) and lay["nested_rgba"] == slice(16, 20)
    lay = capi.aov_layout(capi.make_launch(capi.BF_MODE_TIME, 8, bins=2, bin_width=1.0, film=(2, 1), spp=4), ["position"])
    assert lay["nested"] == slice(8, 14) and lay["chan_px"] == 18
    lay = capi.aov_layout(capi.make_launch(capi.BF_MODE_PATH, 8), ["duv_dx"])
    assert lay["nested"] == slice(7, 7) and lay["nested_rgba"] == slice(7, 11)
    with pytest.raises(ValueError):
        capi.aov_layout(lp, [])


AOV_XML = """
<scene version="2.1.0">
    <integrator type="aov">
        <string name="aovs" value="dd.y:depth,nn:sh_normal"/>
        NESTED
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
RANGE = ('<integrator type="range" name="my_image"><integrator type="pathlength"><integer name="max_depth" value="3"/>'
         '<integer name="rr_depth" value="7"/></integrator><float name="dr" value="0.5"/><integer name="bins" value="3"/></integrator>')
TIME = '<integrator type="time" name="my_image"><integrator type="pathtime"/></integrator>'
PATH = '<integrator type="path" name="my_image"/>'
OWN = ["dd.y", "nn.X", "nn.Y", "nn.Z"]
RGBA = ["my_image.R", "my_image.G", "my_image.B", "my_image.A"]


def _xml(nested, aovs=None):
    x = AOV_XML.replace("NESTED", nested)
    return x if aovs is None else x.replace("dd.y:depth,nn:sh_normal", aovs)


def test_plugin_names_and_launch(mitsuba):
    from beifong_amd.mitsuba.core.xml import load_string
    scene = load_string(_xml(RANGE))
    integ = scene.integrator()
    # aov.cpp:84-150 written out: the AOVs' own names, <child>.<nested aov> ..., <child>.R .G .B .A
    assert integ.aov_names() == OWN + ["my_image.S0.Y", "my_image.S1.Y", "my_image.S2.Y"] + RGBA
    lp = integ.launch_for(scene.sensors()[0])
    assert (lp.mode, lp.bins, lp.max_depth, lp.rr_depth, lp.flags & capi.BF_FLAG_AOV, lp.n_paths) == (capi.BF_MODE_RANGE, 3, 3, 7, 2048, 64)
    lay = capi.aov_layout(lp, ["depth", "sh_normal"])
    assert lay["chan_px"] == 5 + len(integ.aov_names())
    scene = load_string(_xml(PATH))
    assert scene.integrator().aov_names() == OWN + RGBA
    assert scene.integrator().launch_for(scene.sensors()[0]).mode == capi.BF_MODE_PATH
    time_names = load_string(_xml(TIME)).integrator().aov_names()
    assert time_names[:4] == OWN and time_names[-4:] == RGBA and len(time_names) == 4 + 150 + 4
    assert all(n.startswith("my_image.") for n in time_names[4:])
    # every type's channel suffixes
    names = load_string(_xml(PATH, "a:depth, b:position c:uv,d:geo_normal,e:dp_du,f:dp_dv,g:duv_dx,h:duv_dy")).integrator().aov_names()
    assert names[:-4] == ["a", "b.X", "b.Y", "b.Z", "c.U", "c.V", "d.X", "d.Y", "d.Z", "e.X", "e.Y", "e.Z", "f.X", "f.Y", "f.Z",
                          "g.U", "g.V", "h.U", "h.V"]


def test_plugin_error_texts_and_refusals(mitsuba):
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    with pytest.raises(_host.HostError, match=re.escape('Invalid AOV type "normal"!')):
        load_string(_xml(PATH, "nn:normal"))
    for bad in ("depth", "a:depth:x", "a:depth,:uv"):
        with pytest.raises(_host.HostError, match="Invalid AOV specification: require <name>:<type> pair"):
            load_string(_xml(PATH, bad))
    with pytest.raises(_host.HostError, match="more than one nested integrator.*second.*one estimator per path"):
        load_string(_xml(PATH + '<integrator type="path" name="second"/>'))
    with pytest.raises(_host.HostError, match="no nested integrator.*one estimator per path"):
        load_string(_xml(""))
    for fast in (_xml(PATH).replace('<integrator type="aov">', '<integrator type="aov"><boolean name="fast_math" value="true"/>'),
                 _xml(RANGE).replace('<integrator type="pathlength">', '<integrator type="pathlength"><boolean name="fast_math" value="true"/>')):
        with pytest.raises(_host.HostError, match="fast_math"):
            load_string(fast)
    with pytest.raises(_host.HostError, match='nested "moment" integrator is refused'):
        load_string(_xml('<integrator type="moment" name="my_image"><integrator type="path" name="p"/></integrator>'))
    with pytest.raises(_host.HostError, match="Child objects must be of type 'SamplingIntegrator'"):
        load_string(_xml('<bsdf type="diffuse"/>'))


def test_receive_is_refused(mitsuba):
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_host import RECEIVE_SCENE
    xml = RECEIVE_SCENE.replace('<integrator type="pathtimefrequency"/>',
                                '<integrator type="aov"><string name="aovs" value="d:depth"/><integrator type="pathtimefrequency" name="n"/></integrator>')
    assert xml != RECEIVE_SCENE
    scene = load_string(xml)
    with pytest.raises(_host.HostError, match=r"aov: receive\(\) is refused"):
        scene.integrator().receive(scene, scene.receivers()[0])


def test_load_dict_matches_xml(mitsuba):
    from beifong_amd.mitsuba.core import Transform4f
    from beifong_amd.mitsuba.core.xml import load_dict, load_string
    look = Transform4f.look_at([0, 0, 0], [0, -1, 0], [0, 0, 1])
    scene = load_dict({
        "type": "scene",
        "integrator": {"type": "aov", "aovs": "dd.y:depth,nn:sh_normal",
                       "my_image": {"type": "range", "integrator": {"type": "pathlength", "max_depth": 3, "rr_depth": 7}, "dr": 0.5, "bins": 3}},
        "sensor": {"type": "perspective", "to_world": look, "sampler": {"type": "independent", "sample_count": 64},
                   "film": {"type": "hdrfilm", "rfilter": {"type": "box"}, "width": 1, "height": 1}},
        "emitter": {"type": "spot", "intensity": {"type": "spectrum", "value": 10}, "to_world": look},
        "shape": {"type": "rectangle", "to_world": Transform4f.look_at([0, -1, 0], [0, 0, 0], [0, 0, 1]),
                  "bsdf": {"type": "twosided", "bsdf": {"type": "diffuse"}}},
    })
    ref = load_string(_xml(RANGE))
    a, b = scene.integrator().launch_for(scene.sensors()[0]), ref.integrator().launch_for(ref.sensors()[0])
    assert bytes(a) == bytes(b)
    assert scene.integrator().aov_names() == ref.integrator().aov_names()
