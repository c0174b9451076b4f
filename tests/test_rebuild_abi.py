"""CPU-side checks of the device BVH rebuild (bf_scene_rebuild_bvh, bf_scene_read_bvh): the symbols are exported with the
documented signatures, the ABI version and struct sizes did not move, a NULL handle is refused without a device, and the
binding has the methods and the node dtypes.  No GPU is needed."""
import ctypes as C
import os
import re

from beifong_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "beifong_hip.h")


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return capi.load_library()


def test_symbols_and_signatures():
    lib = _lib()
    assert hasattr(lib, "bf_scene_rebuild_bvh") and hasattr(lib, "bf_scene_read_bvh")
    hdr = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    hdr = re.sub(r"\s+", " ", hdr)
    assert "bf_status bf_scene_rebuild_bvh(bf_scene *scene, void *stream);" in hdr
    assert ("bf_status bf_scene_read_bvh(const bf_scene *scene, uint32_t width , void *nodes_out, uint64_t nodes_bytes, "
            "float *tri_rows_out , int32_t *root_child);") in hdr
    assert len(lib.bf_scene_rebuild_bvh.argtypes) == 2
    assert len(lib.bf_scene_read_bvh.argtypes) == 6


def test_abi_version_and_sizes_unchanged():
    lib = _lib()
    assert lib.bf_version() == 5 == capi.BF_ABI_VERSION
    mirrors = [capi.bf_material, capi.bf_shape, capi.bf_emitter, capi.bf_sensor, capi.bf_scene_desc, capi.bf_launch, None, capi.bf_stats,
               capi.bf_scene_info, capi.bf_batch]
    for which, m in enumerate(mirrors):
        want = capi.PATH_RECORD_DTYPE.itemsize if m is None else C.sizeof(m)
        assert lib.bf_abi_sizeof(which) == want, which
    assert lib.bf_abi_sizeof(len(mirrors)) == 0


def test_null_handle_is_invalid():
    lib = _lib()
    assert lib.bf_scene_rebuild_bvh(None, None) == capi.BF_ERR_INVALID
    root = C.c_int32(0)
    assert lib.bf_scene_read_bvh(None, 4, None, 0, None, C.byref(root)) == capi.BF_ERR_INVALID
    assert b"null" in lib.bf_last_error()


def test_binding_surface():
    assert callable(capi.Scene.rebuild_bvh) and callable(capi.Scene.read_bvh)
    assert capi.NODE4_DTYPE.itemsize == 128 and capi.NODE16_DTYPE.itemsize == 512
    assert capi.NODE4_DTYPE.fields["child"][1] == 96            # row 6 of the eight float4
    assert capi.NODE16_DTYPE["c"].subdtype[0].fields["child"][1] == 24
    import inspect
    from beifong_amd import sweep
    assert inspect.signature(sweep.render_deform_sweep).parameters["rebuild_every"].default is None
    from beifong_amd.mitsuba import _host
    assert callable(_host.Scene.rebuild_accel)
