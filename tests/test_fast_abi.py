"""CPU-side checks of the fast-arithmetic mode (BF_FLAG_FAST): the binding's constants are the header's, the library carries
the fast build's launchers, and the host layer's fast_math property parses and sets the flag.  No GPU is needed."""
import ctypes as C
import os
import re

import pytest

from beifong_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "beifong_amd", "host")
HEADER = os.path.join(ROOT, "include", "beifong_hip.h")


def _built():
    if not os.path.exists(capi.LIB_PATH) or not os.path.exists(os.path.join(HOST, "libbeifong_host.so")):
        import __graft_entry__ as g
        g.build()


def test_capi_constants_match_the_header():
    hdr = open(HEADER).read()
    assert int(re.search(r"#define BF_ABI_VERSION (\d+)", hdr).group(1)) == capi.BF_ABI_VERSION == 5
    assert int(re.search(r"\bBF_FLAG_FAST = (\d+)u", hdr).group(1)) == capi.BF_FLAG_FAST == 256
    assert int(re.search(r"\bBF_VARIANT_FAST = (\d+)", hdr).group(1)) == capi.BF_VARIANT_FAST == 4
    flags = [int(v) for v in re.findall(r"\bBF_FLAG_[A-Z_]+ = (\d+)u", hdr)]
    assert len(flags) == len(set(flags)) and all(v & (v - 1) == 0 for v in flags)      # distinct single bits
    assert capi.BF_VARIANT_FAST & (capi.BF_VARIANT_LEAN | capi.BF_VARIANT_WIDE) == 0


def test_library_version_and_fast_launchers():
    _built()
    lib = C.CDLL(capi.LIB_PATH)
    assert lib.bf_version() == 5
    for name in ("bfk_wf_shade", "bfk_wf_trace", "bfk_launch_tail", "bfk_launch_render"):
        assert hasattr(lib, name), name
        assert hasattr(lib, name + "_fast"), name + "_fast"


@pytest.fixture(scope="module")
def mitsuba():
    _built()
    from beifong_amd import mitsuba as m
    m.set_variant("scalar_rgb")
    return m


def test_fast_math_integrator_property(mitsuba):
    from beifong_amd.mitsuba.core.xml import load_dict, load_string
    from tests.test_host import RECEIVE_SCENE, TRANS_RAD_LIKE
    # default false: the launch is the exact one
    scene = load_string(TRANS_RAD_LIKE)
    assert not scene.integrator().launch_for(scene.sensors()[0]).flags & capi.BF_FLAG_FAST
    # XML, on the integrator that renders and on an AOV wrapper around it
    for xml in (TRANS_RAD_LIKE.replace('<integrator type="pathtime"/>', '<integrator type="pathtime"><boolean name="fast_math" value="true"/></integrator>'),
                TRANS_RAD_LIKE.replace('<integrator type="time">', '<integrator type="time"><boolean name="fast_math" value="true"/>')):
        scene = load_string(xml)
        assert scene.integrator().launch_for(scene.sensors()[0]).flags & capi.BF_FLAG_FAST
    # receive()
    scene = load_string(RECEIVE_SCENE.replace('<integrator type="pathtimefrequency"/>',
                                              '<integrator type="pathtimefrequency"><boolean name="fast_math" value="true"/></integrator>'))
    assert scene.integrator().launch_for(scene.receivers()[0]).flags == capi.BF_FLAG_FAST
    # load_dict
    for fast in (False, True):
        sen = {"type": "perspective", "fov": 45, "sampler": {"type": "independent", "sample_count": 64},
               "film": {"type": "hdrfilm", "width": 1, "height": 1, "rfilter": {"type": "box"}}}
        scene = load_dict({"type": "scene", "sensor": sen,
                           "integrator": {"type": "range", "dr": 0.2, "bins": 8, "fast_math": fast, "integrator": {"type": "pathlength"}}})
        assert bool(scene.integrator().launch_for(scene.sensors()[0]).flags & capi.BF_FLAG_FAST) == fast
