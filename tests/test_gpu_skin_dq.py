"""Dual-quaternion skinning on the device (bf_scene_set_skin_mode): a shape in BF_SKIN_DUAL_QUATERNION is posed by
bf_skin_vertices_dq_kernel (or the DQ form of bf_morph_vertices_kernel) from the same bone tables, and from there on is the vertex
update a linear skin is.  Every path is held bit for bit to the oracle on motion.deformed_description(motion.apply_skin_dq(...)),
the numpy statement of the kernel's arithmetic; the rows the device wrote to that statement float for float; histogram cells to
tests/hist_bound.py's fp32 summation bound.  No tolerance of its own."""
import ctypes as C

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, scenes
from beifong_amd.scenedesc import SceneDesc
from tests.bvh_tree_check import check_scene
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _launch_like
from tests.test_gpu_morph import W1, W2, _set, _targets
from tests.test_gpu_motion import _centre, _identity, _same
from tests.test_gpu_skin import (Skin, _attach, _batch_inputs, _bend, _bits, _check_rows, _oracle, _range_scene, _receive_scene,
                                 _rigid_bones, _slots, _strip, _weights)

pytestmark = pytest.mark.gpu
f32 = np.float32
DQ, LINEAR = capi.BF_SKIN_DUAL_QUATERNION, capi.BF_SKIN_LINEAR


def _posed(S, bones):
    return motion.apply_skin_dq(S.rest, S.rest_n, S.index, S.weight, bones)


def _posed_desc(sd, S, bones, xf=None):
    d = motion.deformed_description(sd, {S.k: _posed(S, bones)})
    return d if xf is None else motion.moved_description(d, xf)


def _dq_scene(sd, S):
    g = capi.Scene(sd)
    _attach(g, S)
    g.set_skin_mode(S.k, DQ)
    return g


def _twist(S, deg):
    """bone k turned by k * deg about the bar's own axis (through its joints) on top of a bend: what the mode is for"""
    axis = S.joints[-1] - S.joints[0]
    bones = _bend(S, [30.0, -40.0]).astype(np.float64)
    for k in range(1, S.n_bones):
        t = np.eye(4)
        t[:3] = motion.about(motion.rotation(axis, k * deg), S.joints[0])
        m = np.eye(4)
        m[:3] = bones[k]
        bones[k] = (m @ t)[:3]
    return np.ascontiguousarray(bones, f32)


@pytest.mark.parametrize("case", ["range", "range_normals", "receive_iq"])
def test_pose_then_render(hiplib, case):
    sd, lp, S = _receive_scene() if case == "receive_iq" else _range_scene(case == "range_normals")
    bones = _twist(S, 70.0)
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    _attach(g, S)
    g.set_skin_mode(S.k, DQ)
    _same(g.render(lp, records=True)[1], r0)                 # attaching a skin and setting its mode move nothing
    g.pose_skin(S.k, bones)
    hg, rg, _ = g.render(lp, records=True)
    g.sync()
    _oracle(_posed_desc(sd, S, bones), lp, hg, rg, f"{case} posed by dual quaternions")
    # the same bones blended linearly are another surface
    assert not np.array_equal(_bits(_posed(S, bones)[0]), _bits(motion.apply_skin(S.rest, None, S.index, S.weight, bones)[0]))
    g.set_skin_mode(S.k, LINEAR)
    g.pose_skin(S.k, bones)
    rl = g.render(lp, records=True)[1]
    assert any(not np.array_equal(rl[k], rg[k]) for k in ("L", "aux", "n_rays", "valid"))      # ... and the paths see it
    g.sync()


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
def test_what_the_device_wrote(hiplib, normals):
    sd, lp, S = _range_scene(normals)
    bones = _twist(S, -55.0)
    g = capi.Scene(sd)
    before = check_scene(g)
    _attach(g, S)
    g.set_skin_mode(S.k, DQ)
    g.pose_skin(S.k, bones)
    g.sync()                                                 # no violation: the bound the library derived held
    p, n = _posed(S, bones)
    _check_rows(g, S, p, n)
    check_scene(g, before)                                   # both trees bound the rows they hold
    xf = _identity(sd)
    xf[S.k] = motion.about(motion.rotation([0, 0, 1], 33.0), _centre(sd, S.k), (0.2, 0.1, 0.0))
    g.transform_meshes(xf)
    g.sync()
    _check_rows(g, S, *motion.apply_rigid(p, n, xf[S.k]))
    check_scene(g, before)
    assert float(g.debug_origin_scale()) < 100.0


def _antipodal_bones(n, rng):
    """rigid bones whose quaternions, as the library converts them, are antipodal for about half of the pairs: turns of up to 180
    degrees about any axis"""
    return np.ascontiguousarray(np.stack([motion.about(motion.rotation(rng.normal(size=3), rng.uniform(-180, 180)), rng.uniform(-1, 1, 3),
                                                       rng.uniform(-0.5, 0.5, 3)) for _ in range(n)]), f32)


EDGE = ["nv1", "nv63", "nv257", "nv1000", "one_bone", "bones256", "same_bone", "zero_weight_large_bone", "sign_flip", "pivot_ties"]


@pytest.mark.parametrize("case", EDGE)
def test_kernel_edge_shapes(hiplib, case):
    """test_gpu_skin's edge shapes (all but the affine bones, which this mode refuses), with bones up to 180 degrees apart so that
    lanes take the sign flip, and rows of equal weights; the device's rows against numpy's, bit for bit"""
    rng = np.random.default_rng(EDGE.index(case) + 101)
    nv = {"nv1": 1, "nv63": 63, "nv257": 257, "nv1000": 1000, "bones256": 1000}.get(case, 300)
    n_bones = {"one_bone": 1, "bones256": 256, "zero_weight_large_bone": 4, "sign_flip": 6, "pivot_ties": 5}.get(case, 3)
    with_normals = case in ("nv257", "bones256", "sign_flip")
    v, f = _strip(nv, rng)
    nrm = np.ascontiguousarray(rng.normal(size=(nv, 3)), f32) if with_normals else None
    index = rng.integers(0, n_bones, (nv, 4)).astype(np.uint32)
    weight = _weights(nv, rng)
    bones = _antipodal_bones(n_bones, rng) if case in ("sign_flip", "pivot_ties", "bones256") else _rigid_bones(n_bones, rng)
    if case == "same_bone":
        index[:] = index[:, :1]
    elif case == "zero_weight_large_bone":
        index[:, :2] = rng.integers(0, 3, (nv, 2))
        index[:, 2:] = 3
        weight[:, 2:] = 0.0
        weight[:, 1] = f32(1.0) - weight[:, 0]
        bones[3] = 1e30                                      # finite, not rigid, weighed by no vertex: the table holds the identity for it
    elif case == "pivot_ties":
        weight[0::3] = f32(0.25)
        weight[1::3] = np.array([0.5, 0.5, 0.0, 0.0], f32)
        weight[2::3] = np.array([0.0, 0.375, 0.375, 0.25], f32)      # a tie that slot 0 does not take part in
    if case == "sign_flip":
        d = motion.bone_dual_quaternions(bones)[index.astype(np.int64)][:, :, :4].astype(np.float64)
        dots = np.einsum("vkj,vj->vk", d, d[np.arange(nv), np.argmax(weight, 1)])
        assert ((dots < 0) & (weight > 0)).any(1).mean() > 0.25      # a good share of the lanes flip a slot
    sd = SceneDesc()
    scenes._radar_frontend(sd)
    mat = sd.add_diffuse(0.5)
    pv, pf = meshgen.rectangle_obj()
    sd.add_mesh(pv + f32(3.0), pf, mat)
    sd.add_mesh(v, f, mat, normals=nrm)
    sd.finalize()
    k = len(sd.shapes) - 1
    S = Skin(k, v, nrm, f, index, weight, None, n_bones)
    g = _dq_scene(sd, S)
    before = check_scene(g)
    g.pose_skin(k, bones)
    g.sync()
    p, n = _posed(S, bones)
    assert np.all(np.isfinite(p))
    _check_rows(g, S, p, n)
    check_scene(g, before)
    if case == "zero_weight_large_bone":
        assert float(g.debug_origin_scale()) < 100.0         # a bone no vertex weighs does not enter the bound
    # and the batch's kernel launch (grid y > 1) writes the same vertices into version 1
    lp = capi.make_launch(capi.BF_MODE_RANGE, 256, seed=1, bins=64, bin_width=0.25)
    g2 = _dq_scene(sd, S)
    other = _rigid_bones(n_bones, rng)
    if case == "zero_weight_large_bone":
        other[3] = -1e30
    g2.render_skin_batch(lp, {k: np.ascontiguousarray(np.stack([other, bones]))})
    g2.sync()
    nodes, rows, normals = g2.debug_read_tree(4, 1)
    mine, face = _slots(rows, k)
    assert np.array_equal(_bits(rows[mine][:, :, :3]), _bits(p[f[face]]))
    if n is not None:
        assert np.array_equal(_bits(normals[mine][:, :, :3]), _bits(n[f[face]]))


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normal_deltas"])
def test_morph_ahead_of_the_skin(hiplib, normals):
    sd, lp, S = _range_scene(normals)
    M = _targets(S, normal_deltas=normals)
    bones = _twist(S, 65.0)
    g = capi.Scene(sd)
    _set(g, M)
    _attach(g, S)
    g.set_skin_mode(S.k, DQ)
    g.pose_morph(M.k, W2, bones=bones)
    g.sync()
    p, n = motion.apply_skin_dq(*motion.apply_morph(M.rest, M.rest_n, M.dp, M.dn, W2), S.index, S.weight, bones)
    _check_rows(g, S, p, n)
    check_scene(g)
    g.pose_morph(M.k, W2)                                    # without bones the mode is not looked at
    _check_rows(g, S, *motion.apply_morph(M.rest, M.rest_n, M.dp, M.dn, W2))
    if normals:
        return
    g.pose_morph(M.k, W1, bones=bones)
    hg, rg, _ = g.render(lp, records=True)
    g.sync()
    want = motion.apply_skin_dq(*motion.apply_morph(M.rest, M.rest_n, M.dp, M.dn, W1), S.index, S.weight, bones)
    _oracle(motion.deformed_description(sd, {M.k: want}), lp, hg, rg, "morphed, then skinned by dual quaternions")
    # the morph batch reads the mode too: version 1 of two
    g.render_morph_batch(lp, {M.k: np.ascontiguousarray(np.stack([W2, W1]))},
                         bones={S.k: np.ascontiguousarray(np.stack([_bend(S, [10.0, 10.0]), bones]))})
    g.sync()
    nodes, rows, _ = g.debug_read_tree(4, 1)
    mine, face = _slots(rows, S.k)
    assert np.array_equal(_bits(rows[mine][:, :, :3]), _bits(want[0][S.faces[face]]))


@pytest.mark.parametrize("chunk_mb", [None, "1"], ids=["one_chunk", "chunked"])
def test_batch_with_a_dq_shape_and_a_linear_shape(hiplib, monkeypatch, chunk_mb):
    sd, lp, (S1, S2) = _range_scene(False, second_bar=True)
    n = 4
    b1, xf = _batch_inputs(sd, S1, n)
    b1 = np.ascontiguousarray(np.stack([_twist(S1, 25.0 * (i + 1)) for i in range(n)]))
    b2 = np.ascontiguousarray(np.stack([_bend(S2, [-25.0 * (i + 1)], axis=(0.0, 1.0, 0.2)) for i in range(n)]))
    seeds = [200 + i for i in range(n)]
    g = capi.Scene(sd)
    _attach(g, S1)
    _attach(g, S2)
    g.set_skin_mode(S1.k, DQ)                                # S2 stays linear
    _, r0, _ = g.render(lp, records=True)
    if chunk_mb:
        monkeypatch.setenv("BF_MOTION_BATCH_MB", chunk_mb)   # below one version: one render per chunk
    hb, rb, sb = g.render_skin_batch(lp, {S1.k: b1, S2.k: b2}, transforms=xf, seeds=seeds, records=True)
    if chunk_mb:
        monkeypatch.delenv("BF_MOTION_BATCH_MB")
    assert sb.n_paths == n * lp.n_paths and sb.n_guard == 0
    g.sync()
    ref = g.clone()                                          # the clone has the skins and the modes
    assert (ref.skin_mode(S1.k), ref.skin_mode(S2.k)) == (DQ, LINEAR)
    for i in range(n):
        li = _launch_like(lp, seeds[i], flags=lp.flags)
        ref.pose_skin(S1.k, b1[i])
        ref.pose_skin(S2.k, b2[i])
        ref.transform_meshes(xf[i])
        _same(rb[i], ref.render(li, records=True)[1])
    i = 2
    li = _launch_like(lp, seeds[i], flags=lp.flags)
    want = motion.moved_description(motion.deformed_description(sd, {S1.k: _posed(S1, b1[i])[0],
                                                                     S2.k: motion.apply_skin(S2.rest, None, S2.index, S2.weight, b2[i])[0]}), xf[i])
    ho, ro, so, add = OracleScene(want).render(li, records=True, threads=8, addends=True)
    _same(rb[i], ro)
    assert_fp32_sum(hb[i], add.ref, add.S, add.N, f"mixed batch render {i}", counts=count_channels(li, want))
    _same(g.render(lp, records=True)[1], r0)                 # the handle is as it was
    ref.sync()


def test_skin_sweep_equals_per_pulse(hiplib):
    pytest.importorskip("torch")
    from beifong_amd import sweep
    sd, lp, S = _receive_scene()
    n = 6
    bones = np.ascontiguousarray(np.stack([_twist(S, 20.0 * (i + 1)) for i in range(n)]))
    skins = {S.k: (S.index, S.weight)}
    a = sweep.render_skin_sweep(sd, lp, skins, {S.k: bones}, n_streams=2, dual_quaternion=(S.k,))
    b = sweep.render_skin_sweep(sd, lp, skins, {S.k: bones}, n_streams=2, per_pulse=True, dual_quaternion=(S.k,))
    assert a.shape == b.shape and np.all(a[:, :, 2].sum(1) == b[:, :, 2].sum(1))
    i = 4
    want = _posed_desc(sd, S, bones[i])
    ho, ro, so, add = OracleScene(want).render(lp, records=True, threads=8, addends=True)
    for cube in (a, b):
        assert_fp32_sum(cube[i].reshape(-1), add.ref, add.S, add.N, f"sweep pulse {i}", counts=count_channels(lp, want))
    with pytest.raises(ValueError):
        sweep.render_skin_sweep(sd, lp, skins, {S.k: bones}, dual_quaternion=(S.k + 1,))


def test_mode_plumbing(hiplib):
    sd, lp, S = _range_scene(True)
    bones = _twist(S, 80.0)
    g = capi.Scene(sd)
    assert g.skin_mode(S.k) == LINEAR                        # the default, and it needs no skin
    g.set_skin_mode(S.k, DQ)
    assert g.skin_mode(S.k) == DQ
    _attach(g, S)
    assert g.skin_mode(S.k) == DQ                            # it survives set_skin
    c = g.clone()
    assert c.skin_mode(S.k) == DQ                            # copied at the moment of cloning ...
    c.set_skin_mode(S.k, LINEAR)
    assert g.skin_mode(S.k) == DQ and c.skin_mode(S.k) == LINEAR      # ... and independent afterwards
    g.pose_skin(S.k, bones)
    c.pose_skin(S.k, bones)
    p, n = _posed(S, bones)
    pl, nl = motion.apply_skin(S.rest, S.rest_n, S.index, S.weight, bones)
    _check_rows(g, S, p, n)
    _check_rows(c, S, pl, nl)
    g.set_skin_mode(S.k, LINEAR)                             # setting it moves nothing ...
    _check_rows(g, S, p, n)
    g.pose_skin(S.k, bones)                                  # ... and the next pose is the linear blend, bit for bit
    _check_rows(g, S, pl, nl)
    g.set_skin(S.k, 0)
    assert g.skin_mode(S.k) == LINEAR
    # recomputed normals are those of the DQ-posed surface
    c.set_skin_mode(S.k, DQ)
    c.set_normal_mode(S.k, capi.BF_NORMALS_RECOMPUTE)
    c.pose_skin(S.k, bones)
    _check_rows(c, S, p, motion.vertex_normals_f32(p, S.faces))
    g.sync()
    c.sync()


def test_refusals_leave_the_scene_intact(hiplib):
    pytest.importorskip("torch")
    lib = hiplib
    sd, lp, S = _range_scene(False)
    rect = next(i for i, s in enumerate(sd.shapes) if s.type != capi.BF_SHAPE_MESH)
    bones = _twist(S, 60.0)
    g = _dq_scene(sd, S)
    g.pose_skin(S.k, bones)
    h0, r0, _ = g.render(lp, records=True)
    new_sd = _posed_desc(sd, S, bones)
    _oracle(new_sd, lp, h0, r0, "before the refusals")
    msg = lambda: lib.bf_last_error().decode()
    bp = lambda b: b.ctypes.data_as(C.c_void_p)
    scaled = bones.copy()
    scaled[1, :, :3] = (scaled[1, :, :3].astype(np.float64) @ np.diag([1.5, 0.7, 1.2])).astype(f32)
    sheared = bones.copy()
    sheared[2, :, :3] = np.array([[1.0, 0.4, 0.0], [0.0, 1.0, -0.3], [0.2, 0.0, 0.8]], f32)
    two = np.ascontiguousarray(np.stack([bones, sheared]))
    hist = np.zeros((2, g.channels(lp)), f32)
    sh = np.asarray([S.k], np.uint32)
    ptrs = (C.c_void_p * 1)(two.ctypes.data)

    def refusals():
        assert lib.bf_scene_pose_skin(g.handle, S.k, bp(scaled), None) == capi.BF_ERR_INVALID
        assert "bone 1" in msg() and "rigid" in msg() and "shape %d" % S.k in msg()
        assert lib.bf_render_skin_batch(g.handle, C.byref(lp), 2, None, 1, sh.ctypes.data_as(C.c_void_p), ptrs, 0, None,
                                        hist.ctypes.data_as(C.c_void_p), None, None) == capi.BF_ERR_INVALID
        assert "render 1" in msg() and "bone 2" in msg()
        assert lib.bf_scene_set_skin_mode(g.handle, S.k, 2) == capi.BF_ERR_INVALID and "mode 2" in msg()
        assert lib.bf_scene_set_skin_mode(g.handle, rect, DQ) == capi.BF_ERR_INVALID and "shape %d" % rect in msg()
        mode = C.c_uint32(9)
        assert lib.bf_scene_get_skin_mode(g.handle, rect, C.byref(mode)) == capi.BF_ERR_INVALID and mode.value == 9
        assert lib.bf_scene_set_skin_mode(g.handle, len(sd.shapes), DQ) == capi.BF_ERR_INVALID

    refusals()
    assert g.skin_mode(S.k) == DQ
    _same(g.render(lp, records=True)[1], r0)
    # inside an open rolling sequence: it stays open and flushes what it would have
    seeds = [31, 32, 33, 34]
    seq = _Sequence(g, lp, seeds)
    seq.issue([0, 1])
    refusals()
    seq.issue([2, 3])
    g.flush()
    h, recs = seq.results()
    orc = OracleScene(new_sd)
    for i, seed in enumerate(seeds):
        li = _launch_like(lp, seed)
        ho, ro, so, add = orc.render(li, records=True, threads=8, addends=True)
        _same(recs[i], ro)
        assert_fp32_sum(h[i], add.ref, add.S, add.N, f"rolling render {i}", counts=count_channels(li, new_sd))
    # the linear mode takes the same bones
    g.set_skin_mode(S.k, LINEAR)
    g.pose_skin(S.k, scaled)
    g.sync()
