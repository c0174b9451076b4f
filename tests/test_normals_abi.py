"""Recomputed vertex normals, the surface that needs no GPU: the new entry points exist with the documented
argument counts, the ABI version and the struct sizes did not move, a NULL handle is refused, and the Python layers carry the
new parameters."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from beifong_amd import capi, motion, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"bf_vertex_normals": 5, "bf_scene_set_normal_mode": 3, "bf_scene_get_normal_mode": 3}


def test_symbols_and_argument_counts():
    lib = capi.load_library()
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "beifong_hip.h")).read(), flags=re.S)
    for name, n_args in NEW.items():
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == n_args, name
        m = re.search(r"bf_status %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
    assert re.search(r"BF_NORMALS_GIVEN = 0, BF_NORMALS_RECOMPUTE = 1", hdr)
    assert (capi.BF_NORMALS_GIVEN, capi.BF_NORMALS_RECOMPUTE) == (0, 1)


def test_abi_version_is_still_5():
    lib = capi.load_library()
    assert lib.bf_version() == 5 == capi.BF_ABI_VERSION
    recorded = [44, 248, 208, 416, 480, 80, 16, 192, 72, 24]       # BF_ABI_MATERIAL .. BF_ABI_BATCH, as before this feature
    assert [lib.bf_abi_sizeof(i) for i in range(len(recorded))] == recorded
    assert [C.sizeof(t) for t in capi.ABI_STRUCTS] == recorded
    assert lib.bf_abi_sizeof(len(recorded)) == 0                   # no struct was added


def test_null_handle_is_invalid():
    lib = capi.load_library()
    mode = C.c_uint32(7)
    assert lib.bf_scene_set_normal_mode(None, 0, capi.BF_NORMALS_RECOMPUTE) == capi.BF_ERR_INVALID
    assert b"bf_scene_set_normal_mode" in lib.bf_last_error() and b"null" in lib.bf_last_error()
    assert lib.bf_scene_get_normal_mode(None, 0, C.byref(mode)) == capi.BF_ERR_INVALID
    assert b"bf_scene_get_normal_mode" in lib.bf_last_error() and b"null" in lib.bf_last_error()
    assert mode.value == 7


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_binding_surface():
    g = capi.Scene.__new__(capi.Scene)
    g.lib, g.holder, g.handle, g._borrowed = _NoLibrary(), None, C.c_void_p(1), True
    for bad in (lambda: g.set_normal_mode(-1, capi.BF_NORMALS_RECOMPUTE), lambda: g.set_normal_mode(0, -1), lambda: g.normal_mode(-1)):
        with pytest.raises(ValueError):
            bad()
    assert list(inspect.signature(capi.Scene.set_normal_mode).parameters) == ["self", "shape", "mode"]
    assert list(inspect.signature(capi.Scene.normal_mode).parameters) == ["self", "shape"]
    assert list(inspect.signature(capi.vertex_normals).parameters)[:2] == ["positions", "faces"]
    assert list(inspect.signature(motion.vertex_normals_f32).parameters) == ["positions", "faces"]
    for fn in (sweep.render_deform_sweep, sweep.render_skin_sweep):
        p = inspect.signature(fn).parameters
        assert "recompute_normals" in p and p["recompute_normals"].default is None
    from beifong_amd.mitsuba import _host
    p = inspect.signature(_host.Shape.parameters_changed).parameters
    assert list(p) == ["self", "recompute_normals"] and p["recompute_normals"].default is False
    # one triangle by hand: every corner's normal is the face normal, whatever the angles
    v = np.array([[0, 0, 0], [2, 0, 0], [0, 3, 0]], np.float32)
    n = motion.vertex_normals_f32(v, np.array([[0, 1, 2]], np.uint32))
    assert np.array_equal(n, np.tile(np.float32([0, 0, 1]), (3, 1)))
