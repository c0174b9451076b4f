"""CPU checks of the device-side query entries (include/beifong_hip.h: "plugin-level queries on the device"): the library
exports them, the header and the binding list agree, and a wrong shape or dtype is a ValueError raised by the binding
before any library call (so on any machine, GPU or not)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from beifong_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

QUERY_SYMBOLS = [
    "bf_bsdf_eval_pdf", "bf_bsdf_eval_pdf_device", "bf_bsdf_sample", "bf_bsdf_sample_device",
    "bf_emitter_sample_direction", "bf_emitter_sample_direction_device", "bf_sensor_sample_ray", "bf_sensor_sample_ray_device",
    "bf_ray_intersect_device", "bf_trace_any_device", "bf_eval_microfacet",
]


def _lib_path():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return capi.LIB_PATH


def test_query_symbols_declared_and_listed():
    hdr = open(os.path.join(ROOT, "include", "beifong_hip.h")).read()
    decl = set(re.findall(r"\b(bf_[a-z_]+)\s*\(", hdr))
    for name in QUERY_SYMBOLS:
        assert name in decl, name
        assert name in capi.EXPORTED_SYMBOLS, name
    assert decl == set(capi.EXPORTED_SYMBOLS)


def test_library_exports_query_symbols():
    lib = C.CDLL(_lib_path())
    for name in QUERY_SYMBOLS:
        assert hasattr(lib, name), name


def test_host_layer_exports_device_scene_accessor():
    from beifong_amd.mitsuba import _host
    if not os.path.exists(_host.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    assert hasattr(C.CDLL(_host.LIB_PATH), "bfh_scene_device")


class _Refuse:
    """Stands in for the library: any call is a test failure (the ValueError must come first)."""

    def __getattr__(self, name):
        def call(*a, **k):
            raise AssertionError(f"{name} called: the binding should have refused the arguments first")
        return call


def _scene():
    s = capi.Scene.__new__(capi.Scene)
    s.lib = _Refuse()
    s.holder = None
    s.handle = C.c_void_p(1)
    s._borrowed = True
    return s


F32, F64, U32, I64 = np.float32, np.float64, np.uint32, np.int64


@pytest.mark.parametrize("method,width", [("bsdf_eval_pdf", 6), ("bsdf_sample", 6)])
def test_bsdf_queries_check_shapes_and_dtypes(method, width):
    s = _scene()
    f = getattr(s, method)
    with pytest.raises(ValueError):
        f(np.zeros(4, U32), np.zeros((4, width), F64))            # float64 rows
    with pytest.raises(ValueError):
        f(np.zeros(4, U32), np.zeros((4, width + 1), F32))        # wrong row width
    with pytest.raises(ValueError):
        f(np.zeros(4, U32), np.zeros((4, width - 1), F32))
    with pytest.raises(ValueError):
        f(np.zeros(4, I64), np.zeros((4, width), F32))            # int64 material indices
    with pytest.raises(ValueError):
        f(np.zeros(3, U32), np.zeros((4, width), F32))            # one index per query
    with pytest.raises(ValueError):
        f(np.zeros(4, U32), np.float32(1.0))                      # a scalar


def test_emitter_and_sensor_queries_check_shapes_and_dtypes():
    s = _scene()
    with pytest.raises(ValueError):
        s.emitter_sample_direction(0, np.zeros((4, 4), F32))
    with pytest.raises(ValueError):
        s.emitter_sample_direction(0, np.zeros((4, 5), F64))
    with pytest.raises(ValueError):
        s.sensor_sample_ray(np.zeros((4, 5), F32))
    with pytest.raises(ValueError):
        s.sensor_sample_ray(np.zeros((4, 4), np.float16))


def test_device_forms_take_integer_pointers():
    s = _scene()
    with pytest.raises(ValueError):
        s.bsdf_eval_pdf_device(4, np.zeros(4, U32), 1, 2)
    with pytest.raises(ValueError):
        s.bsdf_sample_device(4, 1, 2.0, 3)
    with pytest.raises(ValueError):
        s.emitter_sample_direction_device(0, 4, "p", 2)
    with pytest.raises(ValueError):
        s.sensor_sample_ray_device(4, 1, None)
    with pytest.raises(ValueError):
        s.ray_intersect_device(4, np.zeros((4, 8), F32), 2)
    with pytest.raises(ValueError):
        s.trace_any_device(4, 1, 2.5)


def test_eval_microfacet_checks_shapes_and_dtypes():
    lib = _Refuse()
    with pytest.raises(ValueError):
        capi.eval_microfacet(0, capi.BF_MF_GGX, .3, .3, True, np.zeros((4, 7), F32), lib=lib)
    with pytest.raises(ValueError):
        capi.eval_microfacet(0, capi.BF_MF_GGX, .3, .3, True, np.zeros((4, 8), F64), lib=lib)


def test_shim_ray_rows():
    from beifong_amd.mitsuba import _host
    r = _host._ray_rows(np.zeros(3, F32), np.array([0, 0, 1], F32))
    assert r.shape == (1, 8) and r.dtype == F32
    assert r[0, 3] == _host.RAY_EPSILON and np.isinf(r[0, 7]) and r[0, 6] == 1
    r = _host._ray_rows(np.zeros((5, 3), F32), np.array([0, 0, 1], F32), mint=0.5, maxt=2.0)
    assert r.shape == (5, 8) and np.all(r[:, 3] == .5) and np.all(r[:, 7] == 2)
    with pytest.raises(ValueError):
        _host._ray_rows(np.zeros((5, 7), F32))
