"""Dual-quaternion skinning (bf_scene_set_skin_mode, bf_bone_dual_quaternions), the parts that need no GPU: the
matrix-to-dual-quaternion conversion of the library against its numpy restatement bit for bit and against scipy; motion.apply_skin_dq,
the fp32 statement of the kernel's arithmetic, against a float64 textbook DQS written here (independent of beifong_amd.motion); what
the mode is for (a twisting joint keeps its volume); and the ABI surface.

The tolerance of the mirror against float64, per coordinate: C 2^-24 (|x|_2 + T / kappa) with C = 64, T the largest |t|_2 over the bones
and kappa the smallest over the vertices of the row's largest weight.  The longest chain of rounded operations from the inputs to an
output coordinate is 1 (the table's rounding to float) + 7 (a component of b) + 8 (|b.real| and the division) + 4 (t) + 5 (rotate) +
6 (the translation and the final sum) = 31 < 64; |x|_2 bounds what the rotation handles and T / kappa the translation."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

from beifong_amd import capi, meshgen, motion, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
C_ULP = 64.0 * 2.0 ** -24
NEW = {"bf_scene_set_skin_mode": 3, "bf_scene_get_skin_mode": 3, "bf_bone_dual_quaternions": 3}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _random_rigid(n, rng, max_deg=180.0):
    return np.ascontiguousarray(np.stack([motion.about(motion.rotation(rng.normal(size=3), rng.uniform(-max_deg, max_deg)),
                                                       rng.uniform(-1, 1, 3), rng.uniform(-0.5, 0.5, 3)) for _ in range(n)]), f32)


def _from_quaternion(q, t=(0.0, 0.0, 0.0)):
    """float32[3, 4] of the rotation of unit quaternion q = (w, x, y, z) and translation t"""
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    r = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    return motion.rigid(r.astype(f32), t)


# ---- the float64 textbook: quaternions (w, x, y, z) ---------------------------------------------------------------------------------
def _qmul(a, b):
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    return np.concatenate([aw * bw - np.sum(av * bv, -1, keepdims=True), aw * bv + bw * av + np.cross(av, bv)], -1)


def _conj(q):
    return q * np.array([1.0, -1.0, -1.0, -1.0])


def _textbook_dq(bones):
    """float64[n, 8]: unit dual quaternions of float32 bones, the rotation by scipy, its scalar part >= 0"""
    b = np.asarray(bones, np.float64).reshape(-1, 3, 4)
    xyzw = Rotation.from_matrix(b[:, :, :3]).as_quat()
    q = np.concatenate([xyzw[:, 3:], xyzw[:, :3]], -1)
    q = np.where(q[:, :1] < 0, -q, q)
    t = np.concatenate([np.zeros((len(b), 1)), b[:, :, 3]], -1)
    return np.concatenate([q, 0.5 * _qmul(t, q)], -1)


def _textbook(positions, normals, index, weight, bones, flips=None):
    """Kavan's DQS in float64: pivot = the slot of largest weight (the first among equals), antipodal slots flipped towards it, blended,
    normalised by the real part's norm, applied as r x r* + 2 vec(e r*).  flips (a list): gets the number of flipped slots of non-zero
    weight."""
    d = _textbook_dq(bones)[np.asarray(index, np.int64)]                      # [nv, 4, 8]
    w = np.asarray(weight, np.float64)
    pivot = d[np.arange(len(w)), np.argmax(np.asarray(weight), 1), :4]
    s = np.where(np.einsum("vkj,vj->vk", d[:, :, :4], pivot) < 0, -1.0, 1.0)
    if flips is not None:
        flips.append(int(((s < 0) & (w > 0)).sum()))
    b = np.einsum("vk,vkj->vj", s * w, d)
    n = np.linalg.norm(b[:, :4], axis=1, keepdims=True)
    r, e = b[:, :4] / n, b[:, 4:] / n

    def rot(v):
        v4 = np.concatenate([np.zeros((len(v), 1)), np.asarray(v, np.float64)], -1)
        return _qmul(_qmul(r, v4), _conj(r))[:, 1:]

    p = rot(positions) + 2.0 * _qmul(e, _conj(r))[:, 1:]
    return p, None if normals is None else rot(normals)


def _tolerance(positions, weight, bones, index):
    used = np.unique(np.asarray(index)[np.asarray(weight) > 0])
    T = float(np.linalg.norm(np.asarray(bones, np.float64).reshape(-1, 3, 4)[used][:, :, 3], axis=1).max())
    kappa = float(np.asarray(weight, np.float64).max(1).min())
    return C_ULP * (np.linalg.norm(np.asarray(positions, np.float64), axis=1, keepdims=True) + T / kappa)


def _assert_mirror(positions, normals, index, weight, bones, flips=None):
    p, n = motion.apply_skin_dq(positions, normals, index, weight, bones)
    pr, nr = _textbook(positions, normals, index, weight, bones, flips)
    assert p.dtype == f32 and p.shape == np.asarray(positions).shape and np.all(np.isfinite(p))
    err = np.abs(p.astype(np.float64) - pr)
    tol = _tolerance(positions, weight, bones, index)
    assert np.all(err <= tol), (err.max(), float((err / tol).max()))
    if normals is not None:
        errn = np.abs(n.astype(np.float64) - nr)
        assert np.all(errn <= C_ULP * np.linalg.norm(np.asarray(normals, np.float64), axis=1, keepdims=True)), errn.max()
    else:
        assert n is None
    return p, n


# ---- the conversion -----------------------------------------------------------------------------------------------------------------
def _branch(m):
    r = np.asarray(m, np.float64)[:, :3]
    return int(np.argmax([(r[0, 0] + r[1, 1]) + r[2, 2], r[0, 0], r[1, 1], r[2, 2]]))


def _against_scipy(bones, dq):
    ref = _textbook_dq(bones)
    for k in range(len(bones)):
        sign = 1.0 if np.dot(ref[k, :4], dq[k, :4]) >= 0 else -1.0
        assert np.abs(sign * ref[k, :4] - dq[k, :4]).max() <= 1e-6, k
        assert np.abs(sign * ref[k, 4:] - dq[k, 4:]).max() <= 1e-6 * (1.0 + np.abs(ref[k, 4:]).max()), k
        assert abs(np.linalg.norm(dq[k, :4].astype(np.float64)) - 1.0) <= 1e-6


def test_conversion_random_bones_bit_for_bit():
    bones = _random_rigid(256, np.random.default_rng(11))
    got, mirror = capi.bone_dual_quaternions(bones), motion.bone_dual_quaternions(bones)
    assert got.shape == mirror.shape == (256, 8) and got.dtype == mirror.dtype == f32
    assert np.array_equal(_bits(got), _bits(mirror))
    assert {_branch(m) for m in bones} == {0, 1, 2, 3}
    _against_scipy(bones, got)


def test_conversion_hits_each_branch():
    named = [("identity", motion.rigid(t=(0.5, -0.25, 2.0)), 0)]
    named += [(f"180 about {a}", motion.about(motion.rotation(a, 180.0), [0.3, -0.2, 0.9], (0.1, 0.2, 0.3)), br)
              for a, br in (((1, 0, 0), 1), ((0, 1, 0), 2), ((0, 0, 1), 3))]
    diag = motion.about(motion.rotation((1, 1, 1), 180.0), [0.3, -0.2, 0.9])
    named.append(("180 about (1, 1, 1)", diag, _branch(diag)))
    bones = np.ascontiguousarray(np.stack([m for _, m, _ in named]), f32)
    got, mirror = capi.bone_dual_quaternions(bones), motion.bone_dual_quaternions(bones)
    assert np.array_equal(_bits(got), _bits(mirror))
    for k, (name, m, br) in enumerate(named):
        assert _branch(m) == br, name
        assert got[k, br] > 0.0, name                         # the component whose square root the branch takes
    assert _branch(diag) in (1, 2, 3)                          # the trace is -1 and the diagonal -1/3: never the trace's branch
    assert np.array_equal(_bits(got[0]), _bits(np.array([1, 0, 0, 0, -0.0, 0.25, -0.125, 1.0], f32)))
    _against_scipy(bones, got)


def test_conversion_refuses_what_is_not_rigid():
    lib = capi.load_library()
    bones = _random_rigid(4, np.random.default_rng(3))
    out = np.full((4, 8), 7.0, f32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    scaled = bones.copy()
    scaled[2, :, :3] = (scaled[2, :, :3].astype(np.float64) @ np.diag([1.5, 0.7, 1.2])).astype(f32)
    nan = bones.copy()
    nan[3, 1, 3] = np.nan
    mirrored = bones.copy()
    mirrored[1, :, 0] *= f32(-1.0)                             # orthogonal, det R = -1
    for bad, word in ((scaled, "bone 2"), (nan, "bone 3"), (mirrored, "bone 1")):
        assert lib.bf_bone_dual_quaternions(4, p(bad), p(out)) == capi.BF_ERR_INVALID
        assert word in lib.bf_last_error().decode(), lib.bf_last_error()
        assert np.all(out == 7.0)                              # nothing was written
        with pytest.raises(capi.BeifongError):
            capi.bone_dual_quaternions(bad)
        with pytest.raises(ValueError, match=word):
            motion.bone_dual_quaternions(bad)
    assert lib.bf_bone_dual_quaternions(4, None, p(out)) == capi.BF_ERR_INVALID
    assert lib.bf_bone_dual_quaternions(0, None, None) == capi.BF_OK
    # the rotations the helpers build pass with room to spare: a product of 300 of them
    rng = np.random.default_rng(5)
    m = np.eye(3, dtype=f32)
    for _ in range(300):
        m = (m @ motion.rotation(rng.normal(size=3), rng.uniform(-180, 180))).astype(f32)
    assert np.abs(m.astype(np.float64).T @ m.astype(np.float64) - np.eye(3)).max() < 1e-5
    capi.bone_dual_quaternions(motion.rigid(m)[None])


# ---- the mirror ---------------------------------------------------------------------------------------------------------------------
def _bar(n_bones=3, radius=0.4):
    v, f, index, weight = meshgen.jointed_bar(n_bones, 8, 6, radius=radius)
    return v, f, meshgen.vertex_normals(v, f), index, weight


def _bend(n_bones, angles, axis=(0.2, 0.1, 1.0), root=None):
    """test_gpu_skin._bend for a bar on the x axis: bone k = bone k - 1 after a turn by angles[k - 1] about the joint at (k, 0, 0)"""
    def m4(m):
        out = np.eye(4)
        out[:3] = np.asarray(m, np.float64).reshape(3, 4)
        return out
    m = np.eye(4) if root is None else m4(root)
    bones = [m[:3].copy()]
    for k in range(1, n_bones):
        m = m @ m4(motion.about(motion.rotation(axis, angles[k - 1]), [float(k), 0.0, 0.0]))
        bones.append(m[:3].copy())
    return np.ascontiguousarray(np.stack(bones), f32)


def test_mirror_against_float64_on_the_bent_bar():
    v, f, n, index, weight = _bar(3)
    root = motion.about(motion.rotation([0, 1, 0], 8.0), [0.0, 0.0, 0.0], (0.1, -0.05, 0.1))
    for angles in ([35.0, -50.0], [-25.0, 60.0], [170.0, -120.0]):
        p, q = _assert_mirror(v, n, index, weight, _bend(3, angles, root=root))
        assert q.dtype == f32 and q.shape == n.shape
    # without normals
    _assert_mirror(v, None, index, weight, _bend(3, [35.0, -50.0]))


def test_mirror_against_float64_on_random_bones_and_weights():
    rng = np.random.default_rng(21)
    nv, n_bones = 600, 16
    v = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (nv, 3)), f32)
    n = np.ascontiguousarray(rng.normal(size=(nv, 3)), f32)
    index = rng.integers(0, n_bones, (nv, 4)).astype(np.uint32)
    w = rng.random((nv, 4)) + 0.05
    weight = np.ascontiguousarray(w / w.sum(1, keepdims=True), f32)
    bones = _random_rigid(n_bones, rng)
    flips = []
    _assert_mirror(v, n, index, weight, bones, flips)
    assert flips[0] > 100                                      # turns of up to 180 degrees: many slots are antipodal to their pivot


@pytest.mark.parametrize("deg,lbs_radius", [(120.0, 0.2), (180.0, 0.0)])
def test_a_twisting_joint_keeps_its_volume(deg, lbs_radius):
    v, f, index, weight = meshgen.jointed_bar(2, 8, 6, radius=0.4)
    bones = np.ascontiguousarray(np.stack([motion.rigid(), motion.about(motion.rotation([1, 0, 0], deg), [1.0, 0.0, 0.0])]), f32)
    rest = np.hypot(v[:, 1].astype(np.float64), v[:, 2].astype(np.float64))
    p, _ = motion.apply_skin_dq(v, None, index, weight, bones)
    assert len(v) == 106
    assert np.abs(np.hypot(p[:, 1].astype(np.float64), p[:, 2].astype(np.float64)) - rest).max() <= 1e-5
    assert np.abs(p[:, 0].astype(np.float64) - v[:, 0]).max() <= 1e-5          # and nothing slides along the axis
    # linear blending: the middle ring (weights 1/2, 1/2) collapses towards the axis
    middle = np.nonzero((weight[:, 0] == 0.5) & (weight[:, 1] == 0.5))[0]
    assert len(middle) == 8 and np.allclose(rest[middle], 0.4, atol=1e-6)
    q, _ = motion.apply_skin(v, None, index, weight, bones)
    assert np.abs(np.hypot(q[middle, 1].astype(np.float64), q[middle, 2].astype(np.float64)) - lbs_radius).max() <= 1e-6


def test_the_same_rigid_bone_in_every_slot_is_that_rigid_motion():
    v, f, n, index, weight = _bar(3)
    rng = np.random.default_rng(31)
    w = rng.random((len(v), 4)) + 0.05
    w = np.ascontiguousarray(w / w.sum(1, keepdims=True), f32)
    m = motion.about(motion.rotation([1, 0.5, 3], 137.0), [1.0, 0.2, -0.3], (0.4, -0.1, 0.7))
    bones = np.ascontiguousarray(np.stack([motion.rigid(t=(9.0, 9.0, 9.0)), m, motion.rigid(t=(-5.0, 0.0, 2.0))]), f32)
    ix = np.ones((len(v), 4), np.uint32)
    p, q = motion.apply_skin_dq(v, n, ix, w, bones)
    pr, qr = motion.apply_rigid(v, n, m)
    # not bit-equal (other operations); both lie within their own rounding of the exact motion, the mirror's being the larger
    tol = _tolerance(v, w, bones, ix)
    assert np.all(np.abs(p.astype(np.float64) - pr) <= tol)
    assert np.all(np.abs(q.astype(np.float64) - qr) <= C_ULP * np.linalg.norm(n.astype(np.float64), axis=1, keepdims=True))
    _assert_mirror(v, n, ix, w, bones)


def test_sign_flip():
    """+100 and -100 degrees about z through the joint: the rotations are 200 degrees apart, so with scalar parts >= 0 the two
    quaternions of every blended vertex are antipodal (dot = cos 100 degrees) and one of them is flipped: the shorter way round."""
    v, f, index, weight = meshgen.jointed_bar(2, 8, 6, radius=0.4)
    joint = [1.0, 0.0, 0.0]
    bones = np.ascontiguousarray(np.stack([motion.about(motion.rotation([0, 0, 1], 100.0), joint),
                                           motion.about(motion.rotation([0, 0, 1], -100.0), joint)]), f32)
    flips = []
    p, _ = _assert_mirror(v, None, index, weight, bones, flips)
    assert flips == [24] and int((weight[:, 0] < 1.0).sum()) == 24
    # the middle ring goes the short way: by 180 degrees, not by 0, and keeps its radius about the z axis through the joint
    middle = np.nonzero((weight[:, 0] == 0.5) & (weight[:, 1] == 0.5))[0]
    assert np.abs(p[middle, :2].astype(np.float64) - (2.0 * np.array(joint[:2]) - v[middle, :2])).max() <= 1e-5
    # ... and bones whose quaternions the library's own conversion leaves antipodal: s_k = -1 inside the mirror itself
    a, b = _from_quaternion([0.5, 0.7, -0.5, 0.1], (0.2, 0.0, -0.1)), _from_quaternion([0.5, -0.5, 0.7, 0.1], (0.0, 0.3, 0.1))
    pair = np.ascontiguousarray(np.stack([a, b]), f32)
    dq = motion.bone_dual_quaternions(pair).astype(np.float64)
    assert np.dot(dq[0, :4], dq[1, :4]) < -0.1
    _assert_mirror(v, None, index, weight, pair)


def test_pivot_ties_pick_slot_0():
    """Three bones with q0 . q1 > 0, q0 . q2 > 0 and q1 . q2 < 0: pivot 0 flips nothing, pivot 1 would flip slot 2 (and 2, slot 1).
    Equal weights pick slot 0, whatever bone it names."""
    qs = [[0.6, 0.5, 0.5, 0.2], [0.3, 0.9, -0.2, 0.1], [0.3, -0.2, 0.9, 0.1]]
    bones = np.ascontiguousarray(np.stack([_from_quaternion(q, t) for q, t in zip(qs, [(0.1, 0, 0), (0, 0.2, 0), (0, 0, 0.3)])]), f32)
    dq = motion.bone_dual_quaternions(bones).astype(np.float64)[:, :4]
    assert dq[0] @ dq[1] > 0.1 and dq[0] @ dq[2] > 0.1 and dq[1] @ dq[2] < -0.1
    x = np.array([[0.3, -1.7, 2.9]] * 6, f32)
    index = np.array([[0, 1, 2, 2], [1, 2, 0, 0], [2, 1, 0, 0], [0, 1, 2, 2], [1, 0, 2, 2], [2, 0, 1, 1]], np.uint32)
    weight = np.array([[0.25] * 4] * 3 + [[0.5, 0.5, 0.0, 0.0]] * 3, f32)
    p, _ = _assert_mirror(x, None, index, weight, bones)

    def by_pivot(row, slot):
        """the float64 blend of `row` with the pivot forced to `slot`"""
        d = _textbook_dq(bones)[index[row].astype(np.int64)]
        s = np.where(d[:, :4] @ d[slot, :4] < 0, -1.0, 1.0)
        b = (s * weight[row].astype(np.float64)) @ d
        r, e = b[:4] / np.linalg.norm(b[:4]), b[4:] / np.linalg.norm(b[:4])
        v4 = np.concatenate([[0.0], x[row].astype(np.float64)])
        return (_qmul(_qmul(r, v4), _conj(r)) + 2.0 * _qmul(e, _conj(r)))[1:]

    for row in range(3):                                       # (1/4, 1/4, 1/4, 1/4)
        assert np.abs(p[row] - by_pivot(row, 0)).max() <= 1e-5
    assert np.abs(p[1] - by_pivot(1, 1)).max() > 1e-2          # slot 1 as the pivot is another vertex
    assert np.abs(p[2] - by_pivot(2, 1)).max() > 1e-2
    for row in range(3, 6):                                    # (1/2, 1/2, 0, 0): either pivot is the same blend up to its sign
        assert np.abs(p[row] - by_pivot(row, 0)).max() <= 1e-5


def test_unused_bones_may_hold_anything_finite():
    v, f, n, index, weight = _bar(3)
    bones = _bend(3, [35.0, -50.0])
    p, q = motion.apply_skin_dq(v, n, index, weight, bones)
    more = np.concatenate([bones, np.full((1, 3, 4), 1e30, f32)])
    ix = index.copy()
    ix[weight == 0] = 3                                        # the zero-weight slots name the bone no vertex weighs
    p2, q2 = motion.apply_skin_dq(v, n, ix, weight, more)
    assert np.array_equal(p, p2) and np.array_equal(q, q2)
    sheared = bones.copy()
    sheared[1, 0, 1] += f32(0.4)
    with pytest.raises(ValueError, match="not rigid"):
        motion.apply_skin_dq(v, n, index, weight, sheared)
    with pytest.raises(ValueError):
        motion.apply_skin_dq(v, n, index, weight, np.concatenate([bones, np.full((1, 3, 4), np.inf, f32)]))


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
def test_symbols_and_argument_counts():
    lib = capi.load_library()
    raw = open(os.path.join(ROOT, "include", "beifong_hip.h")).read()
    assert re.search(r"#define\s+BF_ABI_VERSION\s+5\b", raw)
    hdr = re.sub(r"/\*.*?\*/", " ", raw, flags=re.S)
    for name, n_args in NEW.items():
        assert hasattr(lib, name), name
        assert name in capi.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == n_args, name
        m = re.search(r"bf_status %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
    assert re.search(r"BF_SKIN_LINEAR = 0, BF_SKIN_DUAL_QUATERNION = 1", hdr)
    assert (capi.BF_SKIN_LINEAR, capi.BF_SKIN_DUAL_QUATERNION) == (0, 1)


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
    assert lib.bf_scene_set_skin_mode(None, 0, capi.BF_SKIN_DUAL_QUATERNION) == capi.BF_ERR_INVALID
    assert b"bf_scene_set_skin_mode" in lib.bf_last_error() and b"null" in lib.bf_last_error()
    assert lib.bf_scene_get_skin_mode(None, 0, C.byref(mode)) == capi.BF_ERR_INVALID
    assert b"bf_scene_get_skin_mode" in lib.bf_last_error() and b"null" in lib.bf_last_error()
    assert mode.value == 7


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_binding_surface():
    g = capi.Scene.__new__(capi.Scene)
    g.lib, g.holder, g.handle, g._borrowed = _NoLibrary(), None, C.c_void_p(1), True
    for bad in (lambda: g.set_skin_mode(-1, capi.BF_SKIN_DUAL_QUATERNION), lambda: g.set_skin_mode(0, -1), lambda: g.skin_mode(-1),
                lambda: capi.bone_dual_quaternions(np.zeros((2, 4, 3), f32), lib=_NoLibrary())):
        with pytest.raises(ValueError):
            bad()
    assert list(inspect.signature(capi.Scene.set_skin_mode).parameters) == ["self", "shape", "mode"]
    assert list(inspect.signature(capi.Scene.skin_mode).parameters) == ["self", "shape"]
    assert list(inspect.signature(motion.apply_skin_dq).parameters) == list(inspect.signature(motion.apply_skin).parameters)
    for fn in (sweep.render_skin_sweep, sweep.render_morph_sweep):
        p = inspect.signature(fn).parameters
        assert "dual_quaternion" in p and p["dual_quaternion"].default is None
