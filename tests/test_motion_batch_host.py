"""CPU-side checks of the motion batch (bf_render_motion_batch): the header declares both entries without a new
ABI version, the library exports them, and the binding refuses badly shaped transform tables before it calls the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from beifong_amd import capi, motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "beifong_hip.h")


def test_header_declares_both_entries_at_abi_5():
    hdr = re.sub(r"\s+", " ", open(HEADER).read())
    assert re.search(r"bf_status bf_render_motion_batch_device\(bf_scene \*scene, const bf_launch \*launch, uint32_t n_renders, "
                     r"const uint64_t \*seeds, uint32_t n_shapes, const float \*to_world, float \*hist_dev, "
                     r"bf_path_record \*records_dev, void \*stream, bf_stats \*stats_out\);", hdr)
    assert re.search(r"bf_status bf_render_motion_batch\(bf_scene \*scene, const bf_launch \*launch, uint32_t n_renders, "
                     r"const uint64_t \*seeds, uint32_t n_shapes, const float \*to_world, float \*hist_out, "
                     r"bf_path_record \*records_out, bf_stats \*stats_out\);", hdr)
    assert int(re.search(r"#define BF_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert capi.BF_ABI_VERSION == 5
    assert "BF_MOTION_BATCH_MB" in hdr


def test_library_exports_both_entries():
    for name in ("bf_render_motion_batch_device", "bf_render_motion_batch"):
        assert name in capi.EXPORTED_SYMBOLS
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(capi.LIB_PATH)
    for name in ("bf_render_motion_batch_device", "bf_render_motion_batch"):
        assert hasattr(lib, name)


def _table(n_renders, n_shapes):
    xf = np.zeros((n_renders, n_shapes, 3, 4), np.float32)
    xf[..., :3] = np.eye(3, dtype=np.float32)
    return xf


def test_motion_tables_accepts_and_copies():
    xf = _table(3, 4).astype(np.float64)
    xf[1, 2] = motion.rigid(motion.rotation([0, 0, 1], 30), (1.0, 2.0, 3.0))[:3]
    t, s = capi.motion_tables(xf, 4, seeds=[7, 8, 9])
    assert t.dtype == np.float32 and t.shape == (3, 4, 3, 4) and t.flags["C_CONTIGUOUS"]
    assert np.array_equal(t, xf.astype(np.float32))
    assert s.dtype == np.uint64 and list(s) == [7, 8, 9]
    assert capi.motion_tables(xf, 4)[1] is None


@pytest.mark.parametrize("bad, n, err", [
    (np.zeros((4, 3, 4), np.float32), 4, ValueError),           # one table, not a batch of them
    (np.zeros((2, 4, 4, 4), np.float32), 4, ValueError),        # 4x4 matrices in the batch form
    (np.zeros((2, 3, 3, 4), np.float32), 4, ValueError),        # wrong shape count
    (np.zeros((0, 4, 3, 4), np.float32), 4, ValueError),        # no renders
    (np.zeros((2, 4, 3, 4), np.int32), 4, TypeError),           # not floating point
])
def test_motion_tables_rejects(bad, n, err):
    with pytest.raises(err):
        capi.motion_tables(bad, n)


def test_motion_tables_rejects_seed_count():
    with pytest.raises(ValueError):
        capi.motion_tables(_table(3, 2), 2, seeds=[1, 2])


class _NoRenderLib:
    """Stands in for the library: answers bf_scene_get_info, fails the test if a render entry is reached."""

    def __init__(self, n_shapes):
        self.n_shapes = n_shapes
        self.rendered = False

    def bf_scene_get_info(self, handle, ref):
        ref._obj.n_shapes = self.n_shapes
        return capi.BF_OK

    def bf_launch_channels(self, ref):
        return 8

    def _render(self, *args):
        self.rendered = True
        return capi.BF_OK

    bf_render_motion_batch = bf_render_motion_batch_device = _render


@pytest.mark.parametrize("bad", [np.zeros((2, 5, 3, 4), np.float32), np.zeros((2, 4, 4, 4), np.float32),
                                 np.zeros((4, 3, 4), np.float32)])
def test_scene_refuses_bad_tables_before_the_library(bad):
    sc = capi.Scene.__new__(capi.Scene)
    sc.lib = _NoRenderLib(4)
    sc.handle = C.c_void_p(1)
    launch = capi.make_launch(capi.BF_MODE_RANGE, 64, bins=8, bin_width=0.1)
    with pytest.raises(ValueError):
        sc.render_motion_batch(launch, bad)
    with pytest.raises(ValueError):
        sc.render_motion_batch_device(launch, bad, 0)
    assert not sc.lib.rendered
    sc.handle = None        # (nothing to destroy)
