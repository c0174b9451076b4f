"""CPU-side checks of per-mesh rigid motion (bf_scene_transform_meshes): motion.apply_rigid is the fp32 formula
the header states, the binding builds and checks the transform table without a device, and the library exports the entry."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from beifong_amd import capi, motion

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "beifong_hip.h")
f32 = np.float32


def _cloud(n=20000, seed=0, scale=10.0):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)) * scale).astype(f32)


def _poses():
    return [motion.rigid(motion.rotation([0, 0, 1], 90), (12.0, -3.0, 0.5)),
            motion.rigid(motion.rotation([0, 0, 1], 180)),
            motion.rigid(motion.rotation([1, 2, 3], 37.5), (-1e3, 2e-3, 7.25)),
            motion.about(motion.rotation([0, 1, 0], -15), (5.0, 1.0, 0.0), (0.1, 0.2, 0.3))]


@pytest.mark.parametrize("k", range(4))
def test_apply_rigid_is_close_to_float64(k):
    """Three roundings per row, each of at most half an ulp of a partial sum no larger than |R| |p| + |t|."""
    m = _poses()[k]
    p = _cloud()
    n = motion.rotation([1, 1, 0], 20) @ np.eye(3, dtype=f32)[np.arange(p.shape[0]) % 3].T
    n = np.ascontiguousarray(n.T.astype(f32))
    p2, n2 = motion.apply_rigid(p, n, m)
    assert p2.dtype == f32 and n2.dtype == f32 and p2.shape == p.shape and n2.shape == n.shape
    md = m.astype(np.float64)
    ref = p.astype(np.float64) @ md[:, :3].T + md[:, 3]
    scale = np.abs(p.astype(np.float64)) @ np.abs(md[:, :3]).T + np.abs(md[:, 3])
    assert np.all(np.abs(p2 - ref) <= 4 * 2.0 ** -24 * scale)
    nref = n.astype(np.float64) @ md[:, :3].T
    assert np.all(np.abs(n2 - nref) <= 4 * 2.0 ** -24 * (np.abs(n.astype(np.float64)) @ np.abs(md[:, :3]).T))


@pytest.mark.parametrize("k", range(4))
def test_apply_rigid_is_the_stated_float32_expression(k):
    """Bit for bit: p'_r = fl(fl(fl(fl(m_r0 x) + fl(m_r1 y)) + fl(m_r2 z)) + t_r), evaluated point by point with float32
    scalars (no fused operations anywhere)."""
    m = _poses()[k]
    p = _cloud(500, seed=k)
    n = _cloud(500, seed=10 + k, scale=1.0)
    p2, n2 = motion.apply_rigid(p, n, m)
    for i in range(p.shape[0]):
        for r in range(3):
            a = f32(m[r, 0]) * f32(p[i, 0])
            b = f32(m[r, 1]) * f32(p[i, 1])
            c = f32(m[r, 2]) * f32(p[i, 2])
            v = f32(f32(f32(a + b) + c) + f32(m[r, 3]))
            assert p2[i, r].view(np.uint32) == v.view(np.uint32), (i, r)
            a = f32(m[r, 0]) * f32(n[i, 0])
            b = f32(m[r, 1]) * f32(n[i, 1])
            c = f32(m[r, 2]) * f32(n[i, 2])
            assert n2[i, r].view(np.uint32) == f32(f32(a + b) + c).view(np.uint32), (i, r)


def test_apply_rigid_identity_keeps_the_bits():
    p = _cloud(100)
    p[0] = (-0.0, 0.0, -0.0)
    p2, n2 = motion.apply_rigid(p, None, motion.rigid())
    assert n2 is None and np.array_equal(p2.view(np.uint32), p.view(np.uint32))


def test_rotation_and_about():
    r = motion.rotation([0, 0, 1], 90)
    assert r.dtype == f32 and r.shape == (3, 3)
    assert np.allclose(r @ np.array([1, 0, 0], f32), [0, 1, 0], atol=1e-7)
    assert np.allclose(r.T.astype(np.float64) @ r, np.eye(3), atol=1e-6) and np.linalg.det(r) > 0
    m = motion.about(r, (5.0, 1.0, 0.0), (0.0, 0.0, 2.0))
    q, _ = motion.apply_rigid(np.array([[5.0, 1.0, 0.0], [6.0, 1.0, 0.0]], f32), None, m)
    assert np.allclose(q, [[5.0, 1.0, 2.0], [5.0, 2.0, 2.0]], atol=1e-6)


def test_rigid_table_from_dict_and_array():
    r = motion.rotation([0, 0, 1], 30)
    m4 = np.eye(4, dtype=np.float64)
    m4[:3, :3], m4[:3, 3] = r, (1, 2, 3)
    xf = capi.rigid_table({3: m4, 1: motion.rigid(t=(0, 0, 1))}, 5)
    assert xf.dtype == f32 and xf.shape == (5, 3, 4) and xf.flags.c_contiguous
    assert np.array_equal(xf[0], motion.rigid()) and np.array_equal(xf[2], motion.rigid()) and np.array_equal(xf[4], motion.rigid())
    assert np.array_equal(xf[3], m4[:3].astype(f32)) and xf[1, 2, 3] == 1.0
    arr = np.tile(motion.rigid(), (5, 1, 1)).astype(np.float64)
    out = capi.rigid_table(arr, 5)
    assert out.dtype == f32 and np.array_equal(out, arr.astype(f32))


@pytest.mark.parametrize("bad, n, err", [
    ({5: motion.rigid()}, 5, ValueError),                         # index out of range
    ({-1: motion.rigid()}, 5, ValueError),
    ({0: np.eye(3)}, 5, ValueError),                               # 3x3 is not a transform
    ({0: np.ones((4, 4))}, 5, ValueError),                         # projective last row
    (np.zeros((4, 3, 4), f32), 5, ValueError),                     # wrong shape count
    (np.zeros((5, 4, 4), f32), 5, ValueError),                     # wrong layout
    (np.zeros((5, 3, 4), np.int32), 5, TypeError),                 # not floating point
])
def test_rigid_table_rejects(bad, n, err):
    with pytest.raises(err):
        capi.rigid_table(bad, n)


def test_header_declares_and_library_exports_the_entry():
    hdr = open(HEADER).read()
    assert re.search(r"bf_status bf_scene_transform_meshes\(bf_scene \*scene, uint32_t n_shapes, const float \*to_world, void \*stream\);", hdr)
    assert int(re.search(r"#define BF_ABI_VERSION (\d+)", hdr).group(1)) == 5
    assert "bf_scene_transform_meshes" in capi.EXPORTED_SYMBOLS
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    lib = C.CDLL(capi.LIB_PATH)
    assert hasattr(lib, "bf_scene_transform_meshes") and hasattr(lib, "bfk_launch_rigid")
