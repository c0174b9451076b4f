"""Skinned meshes (bf_scene_set_skin / bf_scene_pose_skin / bf_render_skin_batch), the parts that need no GPU:
motion.apply_skin is the formula of the header evaluated operation by operation in float32, meshgen.jointed_bar is a valid skin,
the four entry points exist with the documented argument counts, the ABI version did not move and a NULL scene is refused."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = {"bf_scene_set_skin": 7, "bf_scene_pose_skin": 4, "bf_render_skin_batch_device": 13, "bf_render_skin_batch": 12}


def _bar():
    v, f, index, weight = meshgen.jointed_bar(3, 8, 6)
    n = meshgen.vertex_normals(v, f)
    return v, f, n, index, weight


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_one_bone_of_weight_one_is_apply_rigid():
    v, f, n, index, weight = _bar()
    m = motion.about(motion.rotation([1, 0.5, 3], 37.0), [1.0, 0.2, -0.3], (0.4, -0.1, 0.7))
    bones = np.stack([motion.rigid(t=(9.0, 9.0, 9.0)), m, motion.rigid(t=(-5.0, 0.0, 2.0))]).astype(f32)
    ix = np.ones((len(v), 4), np.uint32)                       # bone 1 in every slot ...
    w = np.zeros((len(v), 4), f32)
    w[:, 0] = 1.0                                              # ... of which the first has weight 1: p' = fl(1 q) + 0 q + 0 q + 0 q = q
    p, q = motion.apply_skin(v, n, ix, w, bones)
    pr, qr = motion.apply_rigid(v, n, m)
    assert np.array_equal(p, pr) and np.array_equal(q, qr)
    assert p.dtype == f32 and q.dtype == f32 and p.shape == v.shape


def test_identity_bones_reproduce_the_rest_pose():
    v, f, n, index, weight = _bar()
    bones = np.tile(motion.rigid(), (3, 1, 1))
    w = np.zeros((len(v), 4), f32)
    w[:, 0] = 1.0
    p, q = motion.apply_skin(v, n, index, w, bones)
    # np.array_equal, not bit equality: no shortcut is taken for identity bones, so a rest coordinate of -0.0 comes out as
    # fl(fl(-0 + 0) + 0) = +0.0 (the bar has such coordinates: sin / cos of its ring angles times the radius)
    assert np.array_equal(p, v) and np.array_equal(q, n)
    # the blended rows of the bar too: w0 x + w1 x with w0 + w1 = 1 is x up to an ulp or so per product
    p2, _ = motion.apply_skin(v, None, index, weight, bones)
    assert np.allclose(p2, v, rtol=4e-7, atol=1e-30) and _ is None


def test_two_bone_vertex_by_hand():
    x = np.array([[0.3, -1.7, 2.9]], f32)
    nrm = np.array([[0.6, 0.0, -0.8]], f32)
    b = np.stack([motion.about(motion.rotation([0, 0, 1], 25.0), [1.0, 0.0, 0.0], (0.1, 0.2, 0.3)),
                  motion.about(motion.rotation([1, 1, 0], -40.0), [0.0, 2.0, 0.0]), motion.rigid()]).astype(f32)
    ix = np.array([[1, 0, 2, 2]], np.uint32)
    w = np.array([[0.625, 0.375, 0.0, 0.0]], f32)
    p, q = motion.apply_skin(x, nrm, ix, w, b)

    def by_hand(v, with_t):
        out = []
        for r in range(3):
            qs = []
            for k in range(4):
                m = b[ix[0, k]]
                s = f32(f32(f32(m[r, 0] * v[0]) + f32(m[r, 1] * v[1])) + f32(m[r, 2] * v[2]))
                qs.append(f32(s + m[r, 3]) if with_t else s)
            out.append(f32(f32(f32(f32(w[0, 0] * qs[0]) + f32(w[0, 1] * qs[1])) + f32(w[0, 2] * qs[2])) + f32(w[0, 3] * qs[3])))
        return np.array(out, f32)

    assert np.array_equal(_bits(p[0]), _bits(by_hand(x[0], True)))
    assert np.array_equal(_bits(q[0]), _bits(by_hand(nrm[0], False)))
    # and it is a blend: neither bone's own result
    for k in (0, 1):
        assert not np.array_equal(p[0], motion.apply_rigid(x, None, b[k])[0][0])
    with pytest.raises(ValueError):
        motion.apply_skin(x, None, np.array([[0, 1, 2, 3]], np.uint32), w, b)      # bone 3 of 3


@pytest.mark.parametrize("n_bones,n_around,n_along", [(1, 3, 1), (2, 5, 3), (3, 8, 6), (7, 4, 2)])
def test_jointed_bar_is_a_valid_skin(n_bones, n_around, n_along):
    v, f, index, weight = meshgen.jointed_bar(n_bones, n_around, n_along)
    nv = n_around * (n_bones * n_along + 1) + 2
    assert v.shape == (nv, 3) and v.dtype == f32 and index.shape == (nv, 4) and index.dtype == np.uint32
    assert weight.shape == (nv, 4) and weight.dtype == f32
    assert f.shape == (2 * n_around * (n_bones * n_along + 1), 3) and f.dtype == np.uint32 and f.max() == nv - 1
    assert index.max() < n_bones and np.all(weight >= 0.0)
    assert np.all(np.abs(weight.astype(np.float64).sum(1) - 1.0) <= 1e-6)
    assert np.all(weight[:, 2:] == 0.0)                         # two influences
    # bone k owns segment k
    own = np.clip(np.floor(v[:, 0]), 0, n_bones - 1).astype(np.uint32)
    assert np.array_equal(index[:, 0], own) and np.all(weight[:, 0] >= 0.5)
    if n_bones > 1 and n_along > 1:
        blended = (weight[:, 0] < 1.0)
        assert blended.any() and np.all(np.abs(index[blended, 1].astype(int) - index[blended, 0].astype(int)) == 1)
    # closed: every edge is shared by exactly two triangles, in opposite directions
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]).astype(np.int64)
    fwd = set(map(tuple, e))
    assert len(fwd) == len(e) and all((b, a) in fwd for a, b in fwd)
    # outward: the signed volume is that of the prism
    p = v.astype(np.float64)
    vol = np.einsum("ij,ij->i", p[f[:, 0]], np.cross(p[f[:, 1]], p[f[:, 2]])).sum() / 6.0
    assert vol > 0.0


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


def test_abi_version_is_still_5():
    lib = capi.load_library()
    assert lib.bf_version() == 5 == capi.BF_ABI_VERSION
    assert [lib.bf_abi_sizeof(i) for i in range(len(capi.ABI_STRUCTS))] == [C.sizeof(t) for t in capi.ABI_STRUCTS]
    assert lib.bf_abi_sizeof(len(capi.ABI_STRUCTS)) == 0         # no struct was added


def test_null_scene_is_invalid():
    lib = capi.load_library()
    lp = capi.make_launch(capi.BF_MODE_RANGE, 16, seed=1, bins=8, bin_width=1.0)
    buf = (C.c_float * 64)()
    one = (C.c_void_p * 1)(C.addressof(buf))
    sh = (C.c_uint32 * 1)(0)
    assert lib.bf_scene_set_skin(None, 0, 1, buf, None, buf, buf) == capi.BF_ERR_INVALID
    assert lib.bf_scene_set_skin(None, 0, 0, None, None, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_scene_pose_skin(None, 0, buf, None) == capi.BF_ERR_INVALID
    assert lib.bf_render_skin_batch_device(None, C.byref(lp), 1, None, 1, sh, one, 0, None, buf, None, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_render_skin_batch(None, C.byref(lp), 1, None, 1, sh, one, 0, None, buf, None, None) == capi.BF_ERR_INVALID
    assert b"null" in lib.bf_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_binding_refuses_before_the_library():
    from beifong_amd.scenedesc import SceneDesc
    v, f, n, index, weight = _bar()
    sd = SceneDesc()
    sd.add_mesh(v, f, sd.add_diffuse(0.5))
    g = capi.Scene.__new__(capi.Scene)
    g.lib, g.holder, g.handle, g._borrowed = _NoLibrary(), sd, C.c_void_p(1), True
    g._skin_bones = {0: 3}
    bones = np.tile(motion.rigid(), (3, 1, 1))
    lp = capi.make_launch(capi.BF_MODE_RANGE, 16, seed=1, bins=8, bin_width=1.0)
    for bad in (lambda: g.set_skin(0, 3, v.astype(np.float64), index, weight), lambda: g.set_skin(0, 3, v, index.astype(np.int64), weight),
                lambda: g.set_skin(0, 3, v, index, weight.astype(np.float64)), lambda: g.pose_skin(0, bones.astype(np.float64)),
                lambda: g.render_skin_batch(lp, {0: np.tile(bones, (2, 1, 1, 1)).astype(np.float64)})):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: g.set_skin(0, 3, v[:-1], index, weight), lambda: g.set_skin(0, 3, v, index[:-1], weight),
                lambda: g.set_skin(0, 3, v, index, weight[:, :3]), lambda: g.set_skin(-1, 3, v, index, weight),
                lambda: g.pose_skin(0, bones[:2]), lambda: g.pose_skin(0, bones[None]), lambda: g.pose_skin(-1, bones),
                lambda: g.render_skin_batch(lp, {0: bones}), lambda: g.render_skin_batch(lp, {}),
                lambda: g.render_skin_batch(lp, [(0, bones[None]), (0, bones[None])]),
                lambda: g.render_skin_batch(lp, {0: np.tile(bones[:2], (2, 1, 1, 1))}),
                lambda: g.render_skin_batch(lp, {0: np.tile(bones, (2, 1, 1, 1))}, seeds=[1, 2, 3])):
        with pytest.raises(ValueError):
            bad()
    assert capi.bone_array(bones.reshape(3, 12), "bones").shape == (3, 3, 4)
    p = inspect.signature(sweep.render_skin_sweep).parameters
    assert list(p)[:9] == ["sd", "launch", "skins", "bones", "transforms", "n_streams", "per_pulse", "rebuild_every", "classes"]
    assert p["transforms"].default is None and p["n_streams"].default == 2 and p["per_pulse"].default is False
