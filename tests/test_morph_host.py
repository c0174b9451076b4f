"""Morph targets (bf_scene_set_morph / bf_scene_pose_morph / bf_render_morph_batch), the parts that need no GPU:
motion.apply_morph is the formula of the header evaluated operation by operation in float32 (signed zeros and summation order
included), it composes with motion.apply_skin, meshgen.bar_swell_targets is deterministic with the stated overlap, the four entry
points exist with the documented argument counts, the ABI version did not move and a NULL scene is refused."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, sweep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
NEW = {"bf_scene_set_morph": 7, "bf_scene_pose_morph": 5, "bf_render_morph_batch_device": 14, "bf_render_morph_batch": 13}


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _by_hand(rest, deltas, w):
    """p = rest; p_c = fl(p_c + fl(w_k d_k,c)) for k in increasing order, one np.float32 operation at a time"""
    out = np.empty_like(rest)
    for v in range(rest.shape[0]):
        for c in range(3):
            p = f32(rest[v, c])
            for k in range(len(w)):
                p = f32(p + f32(f32(w[k]) * f32(deltas[k, v, c])))
            out[v, c] = p
    return out


def test_apply_morph_against_an_explicit_loop():
    rng = np.random.default_rng(1)
    rest = rng.normal(size=(5, 3)).astype(f32)
    rest_n = rng.normal(size=(5, 3)).astype(f32)
    dp = rng.normal(size=(3, 5, 3)).astype(f32)
    dn = rng.normal(size=(3, 5, 3)).astype(f32)
    w = np.array([0.3, -1.25, 1.7], f32)                      # a negative weight and one above 1
    p, n = motion.apply_morph(rest, rest_n, dp, dn, w)
    assert p.dtype == f32 and n.dtype == f32 and p.shape == rest.shape
    assert np.array_equal(_bits(p), _bits(_by_hand(rest, dp, w)))
    assert np.array_equal(_bits(n), _bits(_by_hand(rest_n, dn, w)))
    # no normal deltas: the rest normals bit for bit; no rest normals: None
    p2, n2 = motion.apply_morph(rest, rest_n, dp, None, w)
    assert np.array_equal(_bits(p2), _bits(p)) and np.array_equal(_bits(n2), _bits(rest_n))
    assert motion.apply_morph(rest, None, dp, None, w)[1] is None
    with pytest.raises(ValueError):
        motion.apply_morph(rest, None, dp, dn, w)                 # normal deltas without rest normals
    with pytest.raises(ValueError):
        motion.apply_morph(rest, None, dp[:, :4], None, w)


def test_signed_zero_takes_no_shortcut():
    rest = np.array([[-0.0, 1.0, -0.0]], f32)
    assert np.all(np.signbit(rest[0, [0, 2]]))
    dp = np.ones((2, 1, 3), f32)
    p, _ = motion.apply_morph(rest, None, dp, None, np.zeros(2, f32))
    # fl(-0 + fl(0 * 1)) = -0 + +0 = +0: every target is evaluated, so the sign of the zero is lost
    assert np.array_equal(p, rest) and not np.any(np.signbit(p))
    assert np.array_equal(_bits(p), _bits(np.array([[0.0, 1.0, 0.0]], f32)))


def test_summation_order_shows():
    # (1 + 2^-24) + 2^-24 in increasing k: each half-ulp addend is rounded away (ties to even) -> 1; the other order adds 2^-23 first
    rest = np.array([[1.0, 1.0, 1.0]], f32)
    h = f32(2.0 ** -24)
    dp = np.array([[[h, h, h]], [[h, h, h]], [[-1.0, -1.0, -1.0]]], f32)
    w = np.ones(3, f32)
    p, _ = motion.apply_morph(rest, None, dp, None, w)
    assert np.all(p == 0.0)                                       # ((1 + h) + h) - 1 = 0 in fp32, in this order
    q, _ = motion.apply_morph(rest, None, dp[::-1], None, w)
    assert np.all(q == f32(2.0 ** -23))                           # ((1 - 1) + h) + h: the order is visible
    assert np.array_equal(_bits(p), _bits(_by_hand(rest, dp, w))) and np.array_equal(_bits(q), _bits(_by_hand(rest, dp[::-1], w)))


def test_composition_with_apply_skin():
    v, f, index, weight = meshgen.jointed_bar(3, 8, 6)
    n = meshgen.vertex_normals(v, f).astype(f32)
    dp = meshgen.bar_swell_targets(v, 3, 5)
    dn = (dp * f32(0.5)).astype(f32)
    w = np.array([0.5, -0.2, 1.5, 0.0, 0.8], f32)
    bones = np.stack([motion.rigid(), motion.about(motion.rotation([0, 0, 1], 30.0), [1.0, 0.0, 0.0]),
                      motion.about(motion.rotation([0, 1, 0], -20.0), [2.0, 0.0, 0.0], (0.1, 0.0, 0.2))]).astype(f32)
    mp, mn = motion.apply_morph(v, n, dp, dn, w)
    p, q = motion.apply_skin(*motion.apply_morph(v, n, dp, dn, w), index, weight, bones)
    pr, qr = motion.apply_skin(mp, mn, index, weight, bones)
    assert np.array_equal(_bits(p), _bits(pr)) and np.array_equal(_bits(q), _bits(qr))
    assert not np.array_equal(p, motion.apply_skin(v, n, index, weight, bones)[0])      # the morph shows through the skin


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


@pytest.mark.parametrize("n_bones,n_targets", [(3, 5), (3, 3), (2, 4), (1, 2)])
def test_bar_swell_targets(n_bones, n_targets):
    v, f, index, weight = meshgen.jointed_bar(n_bones, 8, 6)
    d = meshgen.bar_swell_targets(v, n_bones, n_targets)
    assert d.shape == (n_targets, len(v), 3) and d.dtype == f32 and np.all(np.isfinite(d))
    assert np.array_equal(_bits(d), _bits(meshgen.bar_swell_targets(v.copy(), n_bones, n_targets)))      # deterministic
    moved = np.any(d != 0.0, axis=2)                            # [target, vertex]
    assert np.all(moved.any(1)) and not np.any(moved.all(1))    # each target: some vertices, never all of them
    per_vertex = moved.sum(0)
    assert per_vertex.max() == 2                                # neighbouring targets overlap, and only neighbours do
    for k in range(n_targets - 1):
        assert np.any(moved[k] & moved[k + 1])
    for k in range(n_targets - 2):
        assert not np.any(moved[k] & moved[k + 2])
    # radial: no displacement along the axis, outwards, and the cap centres on the axis stay
    assert np.all(d[:, :, 0] == 0.0) and np.all(d[:, -2:] == 0.0)
    assert np.all(np.einsum("kvc,vc->kv", d.astype(np.float64), v.astype(np.float64) * [0, 1, 1]) >= 0.0)
    with pytest.raises(ValueError):
        meshgen.bar_swell_targets(v, n_bones, 0)


def test_null_scene_is_invalid():
    lib = capi.load_library()
    lp = capi.make_launch(capi.BF_MODE_RANGE, 16, seed=1, bins=8, bin_width=1.0)
    buf = (C.c_float * 64)()
    one = (C.c_void_p * 1)(C.addressof(buf))
    sh = (C.c_uint32 * 1)(0)
    assert lib.bf_scene_set_morph(None, 0, 1, buf, None, buf, None) == capi.BF_ERR_INVALID
    assert lib.bf_scene_set_morph(None, 0, 0, None, None, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_scene_pose_morph(None, 0, buf, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_render_morph_batch_device(None, C.byref(lp), 1, None, 1, sh, one, None, 0, None, buf, None, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_render_morph_batch(None, C.byref(lp), 1, None, 1, sh, one, None, 0, None, buf, None, None) == capi.BF_ERR_INVALID
    assert b"null" in lib.bf_last_error()
    assert lib.bf_render_morph_batch(None, C.byref(lp), 0, None, 1, sh, one, None, 0, None, buf, None, None) == capi.BF_ERR_INVALID
    assert b"n_renders" in lib.bf_last_error()


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def test_binding_refuses_before_the_library():
    from beifong_amd.scenedesc import SceneDesc
    v, f, index, weight = meshgen.jointed_bar(3, 8, 6)
    dp = meshgen.bar_swell_targets(v, 3, 5)
    sd = SceneDesc()
    sd.add_mesh(v, f, sd.add_diffuse(0.5))
    g = capi.Scene.__new__(capi.Scene)
    g.lib, g.holder, g.handle, g._borrowed = _NoLibrary(), sd, C.c_void_p(1), True
    g._morph_targets, g._skin_bones = {0: 5}, {0: 3}
    w = np.zeros(5, f32)
    bones = np.tile(motion.rigid(), (3, 1, 1))
    lp = capi.make_launch(capi.BF_MODE_RANGE, 16, seed=1, bins=8, bin_width=1.0)
    for bad in (lambda: g.set_morph(0, 5, v.astype(np.float64), dp), lambda: g.set_morph(0, 5, v, dp.astype(np.float64)),
                lambda: g.set_morph(0, 5, v, dp, delta_normals=dp.astype(np.float64)), lambda: g.pose_morph(0, w.astype(np.float64)),
                lambda: g.pose_morph(0, w, bones=bones.astype(np.float64)), lambda: g.render_morph_batch(lp, {0: np.zeros((2, 5))})):
        with pytest.raises(TypeError):
            bad()
    for bad in (lambda: g.set_morph(0, 5, v[:-1], dp), lambda: g.set_morph(0, 5, v, dp[:4]), lambda: g.set_morph(0, 5, v, dp[:, :-1]),
                lambda: g.set_morph(-1, 5, v, dp), lambda: g.pose_morph(0, w[:4]), lambda: g.pose_morph(0, w[None]),
                lambda: g.pose_morph(-1, w), lambda: g.pose_morph(0, w, bones=bones[:2]),
                lambda: g.render_morph_batch(lp, {0: w}), lambda: g.render_morph_batch(lp, {}),
                lambda: g.render_morph_batch(lp, [(0, w[None]), (0, w[None])]),
                lambda: g.render_morph_batch(lp, {0: np.zeros((2, 4), f32)}),
                lambda: g.render_morph_batch(lp, {0: np.zeros((2, 5), f32)}, bones={1: np.tile(bones, (2, 1, 1, 1))}),
                lambda: g.render_morph_batch(lp, {0: np.zeros((2, 5), f32)}, bones={0: np.tile(bones, (3, 1, 1, 1))}),
                lambda: g.render_morph_batch(lp, {0: np.zeros((2, 5), f32)}, seeds=[1, 2, 3])):
        with pytest.raises(ValueError):
            bad()
    p = inspect.signature(sweep.render_morph_sweep).parameters
    assert list(p)[:12] == ["sd", "launch", "morphs", "weights", "skins", "bones", "transforms", "n_streams", "per_pulse", "rebuild_every",
                            "classes", "recompute_normals"]
    assert p["skins"].default is None and p["bones"].default is None and p["per_pulse"].default is False and p["rebuild_every"].default is None
    assert p["classes"].default is None and p["recompute_normals"].default == ()
