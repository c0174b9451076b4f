"""Morph targets (bf_scene_set_morph, bf_scene_pose_morph, bf_render_morph_batch): the device computes the vertices of a
mesh from a rest shape, dense per-target deltas and a few weights, optionally skins them in the same kernel, then treats them as a
vertex update.  Every path is held bit for bit to the oracle on motion.deformed_description(motion.apply_morph(...)) (composed with
motion.apply_skin where bones are given), the numpy statement of the arithmetic; histogram cells to tests/hist_bound.py's fp32
summation bound.  No tolerance of its own, except where two fp32 atomic sums of the same addends are compared with each other
(test_flags_pass_through states its bound).  Scenes and sizes are tests/test_gpu_skin.py's."""
import collections
import ctypes as C

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, scenes
from beifong_amd.scenedesc import SceneDesc, Transform4f as T
from tests import hist_bound
from tests.bvh_tree_check import check_scene
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _launch_like
from tests.test_gpu_deform import _verts
from tests.test_gpu_motion import _centre, _identity, _same, _with_flags
from tests.test_gpu_skin import (N_PATHS, Skin, _attach, _bend, _bits, _check_rows, _oracle, _range_scene, _receive_scene, _rigid_bones,
                                 _slots, _strip, _weights)

pytestmark = pytest.mark.gpu
f32 = np.float32
N_TARGETS = 5

Morph = collections.namedtuple("Morph", "k rest rest_n faces dp dn")


def _targets(S, n_targets=N_TARGETS, amplitude=0.15, normal_deltas=False):
    """meshgen.bar_swell_targets for the placed bar of skin-test scene S: the bar's own frame is recovered from its joints, the
    radial deltas are turned back into the scene's; normal deltas, where wanted, are some smooth per-vertex field (any finite one
    is a valid input)"""
    j0, j1 = S.joints[0], S.joints[-1]
    length = np.linalg.norm(j1 - j0)
    u = (j1 - j0) / length
    e1 = np.cross(u, [0.3, 0.5, 0.8])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(u, e1)
    q = S.rest.astype(np.float64) - j0
    local = np.stack([q @ u * (S.n_bones / length), q @ e1, q @ e2], -1)
    local[np.hypot(local[:, 1], local[:, 2]) < 1e-6, 1:] = 0.0      # the cap centres lie on the axis: float32 placement left a residue
    d = meshgen.bar_swell_targets(local, S.n_bones, n_targets, amplitude).astype(np.float64)
    dp = np.ascontiguousarray((d[..., 1:2] * e1 + d[..., 2:3] * e2).astype(f32))
    dn = None
    if normal_deltas:
        assert S.rest_n is not None
        dn = np.ascontiguousarray((f32(2.0) * dp + f32(0.05) * np.sin(S.rest[None] * f32(3.0) + np.arange(n_targets, dtype=f32)[:, None, None])).astype(f32))
    return Morph(S.k, S.rest, S.rest_n, S.faces, dp, dn)


W1 = np.array([0.9, -0.6, 1.4, 0.0, 0.7], f32)                 # a negative weight, one above 1 and a zero
W2 = np.array([-0.3, 1.0, 0.25, 1.2, -0.8], f32)


def _set(g, M):
    g.set_morph(M.k, M.dp.shape[0], M.rest, M.dp, rest_normals=M.rest_n, delta_normals=M.dn)


def _morphed(M, w, S=None, bones=None):
    """the numpy statement: apply_morph, and apply_skin behind it where bones are given"""
    p, n = motion.apply_morph(M.rest, M.rest_n, M.dp, M.dn, w)
    return (p, n) if bones is None else motion.apply_skin(p, n, S.index, S.weight, bones)


def _desc(sd, M, w, S=None, bones=None, xf=None):
    d = motion.deformed_description(sd, {M.k: _morphed(M, w, S, bones)})
    return d if xf is None else motion.moved_description(d, xf)


@pytest.mark.parametrize("case", ["range", "range_normals", "range_normal_deltas", "receive_iq"])
def test_pose_then_render(hiplib, case):
    sd, lp, S = _receive_scene() if case == "receive_iq" else _range_scene(case != "range")
    M = _targets(S, normal_deltas=case == "range_normal_deltas")
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    _set(g, M)
    _attach(g, S)
    _same(g.render(lp, records=True)[1], r0)                 # attaching a morph (and a skin) moves nothing
    g.pose_morph(M.k, W1)
    hg, rg, _ = g.render(lp, records=True)
    g.sync()
    assert not np.array_equal(rg["L"], r0["L"])              # the pose shows
    # some vertices are moved by two targets, and every target leaves some vertices alone
    moved = np.any(M.dp != 0.0, axis=2)
    assert moved.sum(0).max() == 2 and np.all(moved.sum(1) < len(M.rest)) and np.all(moved.any(1))
    p, n = _morphed(M, W1)
    if M.rest_n is not None and M.dn is None:
        assert np.array_equal(_bits(n), _bits(M.rest_n))
    ro = _oracle(_desc(sd, M, W1), lp, hg, rg, f"{case} morphed")
    # bones on top: morphed, then skinned
    bones = _bend(S, [35.0, -50.0], root=motion.about(motion.rotation([0, 1, 0], 8.0), S.joints[0], (0.1, -0.05, 0.1)))
    g.pose_morph(M.k, W1, bones=bones)
    hg, rg, _ = g.render(lp, records=True)
    g.sync()
    assert not np.array_equal(rg["L"], ro["L"])
    _oracle(_desc(sd, M, W1, S, bones), lp, hg, rg, f"{case} morphed and skinned")


@pytest.mark.parametrize("bones", [False, True], ids=["morph", "morph_skin"])
@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
def test_what_the_device_wrote(hiplib, normals, bones):
    sd, lp, S = _range_scene(normals)
    M = _targets(S, normal_deltas=normals)
    b = _bend(S, [-25.0, 60.0]) if bones else None
    g = capi.Scene(sd)
    before = check_scene(g)
    _set(g, M)
    _attach(g, S)
    g.pose_morph(M.k, W2, bones=b)
    g.sync()                                                 # no violation: the bound the library computed held
    p, n = _morphed(M, W2, S, b)
    _check_rows(g, S, p, n)
    check_scene(g, before)                                   # both trees bound the rows they hold
    # under a pose of the handle: rigid_apply of the morphed vertices
    xf = _identity(sd)
    xf[S.k] = motion.about(motion.rotation([0, 0, 1], 33.0), _centre(sd, S.k), (0.2, 0.1, 0.0))
    g.transform_meshes(xf)
    g.sync()
    _check_rows(g, S, *motion.apply_rigid(p, n, xf[S.k]))
    check_scene(g, before)
    assert float(g.debug_origin_scale()) < 100.0


EDGE = ["nv1_t1", "nv63_t5", "nv256_t5", "nv257_t256", "nv1000_t5", "zero_weight_large_target", "signed_weights", "cancel",
        "normals_no_deltas", "skin_bones256"]


@pytest.mark.parametrize("case", EDGE)
def test_kernel_edge_shapes(hiplib, case):
    """the grid's ragged end, one block and several, one target, a count that is no multiple of the unroll factor and the largest,
    and what a weight may be; the device's rows against numpy's, bit for bit, as a pose and as version 1 of a two-render batch"""
    rng = np.random.default_rng(EDGE.index(case) + 1)
    nv = {"nv1_t1": 1, "nv63_t5": 63, "nv256_t5": 256, "nv257_t256": 257, "nv1000_t5": 1000, "skin_bones256": 1000}.get(case, 300)
    nt = {"nv1_t1": 1, "nv257_t256": 256, "cancel": 2}.get(case, 5)
    with_normals = case in ("nv257_t256", "normals_no_deltas", "skin_bones256", "nv63_t5")
    normal_deltas = with_normals and case != "normals_no_deltas"
    v, f = _strip(nv, rng)
    nrm = np.ascontiguousarray(rng.normal(size=(nv, 3)), f32) if with_normals else None
    scale = 4.0 / nt
    dp = np.ascontiguousarray(rng.uniform(-scale, scale, (nt, nv, 3)), f32)
    dn = np.ascontiguousarray(rng.normal(size=(nt, nv, 3)), f32) if normal_deltas else None
    w = np.ascontiguousarray(rng.uniform(0.0, 1.0, nt), f32)
    other = np.ascontiguousarray(rng.uniform(0.0, 1.0, nt), f32)
    if case == "zero_weight_large_target":
        dp[3] = 1e30                                         # large but finite: fl(0 d) = 0 whatever d is
        w[3] = other[3] = 0.0
    elif case == "signed_weights":
        w[:] = [-1.5, 2.25, -0.125, 3.0, 1.0]
    elif case == "cancel":
        dp[1] = -dp[0]
        w[:] = 0.75                                          # fl(fl(r + t) - t): the two targets cancel exactly in exact arithmetic only
    S = None
    bones = bones_other = None
    if case == "skin_bones256":
        S = Skin(None, v, nrm, f, rng.integers(0, 256, (nv, 4)).astype(np.uint32), _weights(nv, rng), None, 256)
        bones, bones_other = _rigid_bones(256, rng), _rigid_bones(256, rng)
    sd = SceneDesc()
    scenes._radar_frontend(sd)
    mat = sd.add_diffuse(0.5)
    pv, pf = meshgen.rectangle_obj()
    sd.add_mesh(pv + f32(3.0), pf, mat)
    sd.add_mesh(v, f, mat, normals=nrm)
    sd.finalize()
    k = len(sd.shapes) - 1
    M = Morph(k, v, nrm, f, dp, dn)
    R = Skin(k, v, nrm, f, None, None, None, 0)              # what _check_rows reads: k and faces
    g = capi.Scene(sd)
    before = check_scene(g)
    _set(g, M)
    if S is not None:
        g.set_skin(k, 256, v, S.index, S.weight, rest_normals=nrm)
    g.pose_morph(k, w, bones=bones)
    g.sync()
    p, n = _morphed(M, w, S, bones)
    assert np.all(np.isfinite(p))
    if case == "cancel":
        assert not np.array_equal(_bits(p), _bits(v))        # the roundings of the first sum stay
    if case == "normals_no_deltas":
        assert np.array_equal(_bits(n), _bits(nrm))
    _check_rows(g, R, p, n)
    check_scene(g, before)
    if case == "zero_weight_large_target":
        assert float(g.debug_origin_scale()) < 100.0         # a target of weight zero does not enter the bound
    # and the batch's kernel launch (grid y > 1) writes the same vertices into version 1
    lp = capi.make_launch(capi.BF_MODE_RANGE, 256, seed=1, bins=64, bin_width=0.25)
    g2 = capi.Scene(sd)
    _set(g2, M)
    if S is not None:
        g2.set_skin(k, 256, v, S.index, S.weight, rest_normals=nrm)
    g2.render_morph_batch(lp, {k: np.ascontiguousarray(np.stack([other, w]))},
                          bones=None if S is None else {k: np.ascontiguousarray(np.stack([bones_other, bones]))})
    g2.sync()
    nodes, rows, normals = g2.debug_read_tree(4, 1)
    mine, face = _slots(rows, k)
    assert np.array_equal(_bits(rows[mine][:, :, :3]), _bits(p[f[face]]))
    if n is not None:
        assert np.array_equal(_bits(normals[mine][:, :, :3]), _bits(n[f[face]]))


def test_interleaved_updates_the_last_one_wins(hiplib):
    """pose_morph, update_vertices, pose_skin and pose_morph interleaved, under a pose of the handle; a rebuild keeps the morph"""
    sd, lp, S = _range_scene(True)
    M = _targets(S, normal_deltas=True)
    bones = _bend(S, [40.0, -30.0])
    xf = _identity(sd)
    xf[S.k] = motion.about(motion.rotation([0, 0, 1], 50.0), _centre(sd, S.k), (0.3, 0.4, 0.0))
    g = capi.Scene(sd)
    _set(g, M)
    _attach(g, S)
    g.transform_meshes(xf)
    g.pose_morph(M.k, W1)
    h, r, _ = g.render(lp, records=True)
    r1 = _oracle(_desc(sd, M, W1, xf=xf), lp, h, r, "pose_morph")
    moved = (S.rest + f32(0.25)).astype(f32)
    g.update_vertices(S.k, moved, S.rest_n)
    h, r, _ = g.render(lp, records=True)
    _oracle(motion.moved_description(motion.deformed_description(sd, {S.k: (moved, S.rest_n)}), xf), lp, h, r, "update after a morph pose")
    g.pose_skin(S.k, bones)
    h, r, _ = g.render(lp, records=True)
    _oracle(motion.moved_description(motion.deformed_description(sd, {S.k: motion.apply_skin(S.rest, S.rest_n, S.index, S.weight, bones)}), xf),
            lp, h, r, "pose_skin after it")
    g.pose_morph(M.k, W2, bones=bones)                       # starts from the morph's rest arrays, not from the base
    h, r, _ = g.render(lp, records=True)
    r2 = _oracle(_desc(sd, M, W2, S, bones, xf), lp, h, r, "pose_morph with bones after it")
    # a rebuild keeps the morph valid and renders the same records
    g.rebuild_bvh()
    _same(g.render(lp, records=True)[1], r2)
    g.pose_morph(M.k, W1)
    _same(g.render(lp, records=True)[1], r1)
    check_scene(g)
    g.sync()


def test_clones_copy_on_write(hiplib):
    sd, lp, S = _range_scene(False)
    M = _targets(S)
    g = capi.Scene(sd)
    _set(g, M)
    c = g.clone()                                            # shares the morph
    _, r0, _ = g.render(lp, records=True)
    c.pose_morph(M.k, W1)
    hc, rc, _ = c.render(lp, records=True)
    _same(g.render(lp, records=True)[1], r0)                 # the original is untouched
    ra = _oracle(_desc(sd, M, W1), lp, hc, rc, "clone posed")
    g.pose_morph(M.k, W2)
    _same(c.render(lp, records=True)[1], ra)                 # and the reverse
    hg, rg, _ = g.render(lp, records=True)
    rb = _oracle(_desc(sd, M, W2), lp, hg, rg, "original posed")
    # a new morph on the clone alone: the original keeps the one it has
    one = Morph(M.k, M.rest, None, M.faces, np.ascontiguousarray(np.tile(f32([0.0, 0.5, 0.2]), (1, len(M.rest), 1))), None)
    _set(c, one)
    lone = np.array([1.0], f32)
    c.pose_morph(M.k, lone)
    hc, rc, _ = c.render(lp, records=True)
    _oracle(_desc(sd, one, lone), lp, hc, rc, "clone with its own morph")
    g.pose_morph(M.k, W1)
    _same(g.render(lp, records=True)[1], ra)
    g.close()
    _same(c.render(lp, records=True)[1], rc)
    assert not np.array_equal(rb["L"], ra["L"])


def test_rolling_sequence_around_a_pose(hiplib):
    pytest.importorskip("torch")
    sd, lp, S = _range_scene(False)
    M = _targets(S)
    g = capi.Scene(sd)
    _set(g, M)
    seeds = [21, 22, 23, 24]
    seq = _Sequence(g, lp, seeds)
    seq.issue([0, 1])
    g.pose_morph(M.k, W1)                                    # finishes the open sequence first
    seq.issue([2, 3])
    g.flush()
    h, recs = seq.results()
    new_sd = _desc(sd, M, W1)
    old, new = OracleScene(sd), OracleScene(new_sd)
    for i, seed in enumerate(seeds):
        li = _launch_like(lp, seed)
        ho, ro, so, add = (old if i < 2 else new).render(li, records=True, threads=8, addends=True)
        _same(recs[i], ro)
        assert_fp32_sum(h[i], add.ref, add.S, add.N, f"rolling render {i}", counts=count_channels(li, sd if i < 2 else new_sd))


K = 8


def _batch_inputs(sd, S, n=K):
    """n weight rows and bone tables that differ from render to render, and a rigid table per render that moves the bar and the bus"""
    i = np.arange(n, dtype=np.float64)[:, None]
    weights = np.ascontiguousarray((1.2 * np.sin(0.7 * i + np.arange(N_TARGETS)) - 0.1 * i / n).astype(f32))
    bones = np.ascontiguousarray(np.stack([_bend(S, [10.0 * (j + 1), -60.0 + 13.0 * j], root=motion.rigid(t=(0.02 * j, 0.0, 0.01 * j)))
                                           for j in range(n)]))
    xf = np.tile(_identity(sd)[None], (n, 1, 1, 1))
    bus = next((j for j, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH and j != S.k), S.k)      # (the receive scene has none)
    for j in range(n):
        xf[j, bus] = motion.about(motion.rotation([0, 0, 1], 9.0 * (j + 1)), _centre(sd, bus), (0.05 * j, -0.03 * j, 0.0))
        xf[j, S.k] = motion.about(motion.rotation([0, 0, 1], -7.0 * j), _centre(sd, S.k), (0.0, 0.04 * j, 0.0))
    return weights, bones, xf.astype(f32)


@pytest.mark.parametrize("with_xf", [True, False], ids=["to_world", "no_to_world"])
@pytest.mark.parametrize("chunk_mb", [None, "1"], ids=["one_chunk", "chunked"])
def test_batch_equals_pose_transform_render(hiplib, monkeypatch, chunk_mb, with_xf):
    sd, lp, S = _range_scene(True)
    M = _targets(S, normal_deltas=True)
    weights, bones, xf = _batch_inputs(sd, S)
    if not with_xf:
        xf = None
    seeds = [100 + i for i in range(K)]
    g = capi.Scene(sd)
    _set(g, M)
    c = g.clone()
    _, r0, _ = g.render(lp, records=True)
    if chunk_mb:
        monkeypatch.setenv("BF_MOTION_BATCH_MB", chunk_mb)   # below one version: one render per chunk
    hb, rb, sb = g.render_morph_batch(lp, {M.k: weights}, transforms=xf, seeds=seeds, records=True)
    if chunk_mb:
        monkeypatch.delenv("BF_MOTION_BATCH_MB")
    assert sb.n_paths == K * lp.n_paths and sb.n_guard == 0
    g.sync()
    ref = capi.Scene(sd)
    _set(ref, M)
    for i in range(K):
        li = _launch_like(lp, seeds[i], flags=lp.flags)
        ref.pose_morph(M.k, weights[i])
        if xf is not None:
            ref.transform_meshes(xf[i])
        _same(rb[i], ref.render(li, records=True)[1])
    for i in (0, 5):
        li = _launch_like(lp, seeds[i], flags=lp.flags)
        want = _desc(sd, M, weights[i], xf=None if xf is None else xf[i])
        ho, ro, so, add = OracleScene(want).render(li, records=True, threads=8, addends=True)
        _same(rb[i], ro)
        assert_fp32_sum(hb[i], add.ref, add.S, add.N, f"morph batch render {i}", counts=count_channels(li, want))
    # the handle and its clone are as they were
    _same(g.render(lp, records=True)[1], r0)
    _same(c.render(lp, records=True)[1], r0)


def test_two_morphed_shapes_one_of_them_skinned(hiplib):
    sd, lp, (S1, S2) = _range_scene(False, second_bar=True)
    M1, M2 = _targets(S1), _targets(S2, n_targets=3)
    n = 3
    w1 = np.ascontiguousarray(np.stack([W1, W2, f32(0.5) * W1]))
    w2 = np.ascontiguousarray(np.array([[1.0, -0.5, 0.3], [0.2, 0.9, -1.1], [1.5, 0.0, 0.6]], f32))
    b1 = np.ascontiguousarray(np.stack([_bend(S1, [20.0 * (i + 1), -15.0 * (i + 1)]) for i in range(n)]))
    g = capi.Scene(sd)
    _set(g, M1)
    _set(g, M2)
    _attach(g, S1)
    hb, rb, _ = g.render_morph_batch(lp, {M2.k: w2, M1.k: w1}, bones={M1.k: b1}, records=True)
    g.sync()
    ref = capi.Scene(sd)
    _set(ref, M1)
    _set(ref, M2)
    _attach(ref, S1)
    for i in range(n):
        want = motion.deformed_description(sd, {M1.k: _morphed(M1, w1[i], S1, b1[i])[0], M2.k: _morphed(M2, w2[i])[0]})
        _oracle(want, lp, hb[i], rb[i], f"two morphs, render {i}")
        ref.pose_morph(M1.k, w1[i], bones=b1[i])
        ref.pose_morph(M2.k, w2[i])
        _same(rb[i], ref.render(lp, records=True)[1])
    # one of the two alone: the other stays at the handle's base
    _, r1, _ = g.render_morph_batch(lp, {M2.k: w2[:1]}, records=True)
    _oracle(motion.deformed_description(sd, {M2.k: _morphed(M2, w2[0])[0]}), lp, None, r1[0], "one of two")


@pytest.mark.parametrize("bones", [False, True], ids=["morph", "morph_skin"])
def test_recomputed_normals(hiplib, bones):
    """under BF_NORMALS_RECOMPUTE a pose and every batch version carry vertex_normals_f32 of the final positions"""
    sd, lp, S = _range_scene(True)
    M = _targets(S, normal_deltas=True)
    weights, btab, xf = _batch_inputs(sd, S, 3)
    b = (lambda i: btab[i]) if bones else (lambda i: None)
    g = capi.Scene(sd)
    _set(g, M)
    _attach(g, S)
    g.set_normal_mode(S.k, capi.BF_NORMALS_RECOMPUTE)
    g.pose_morph(M.k, weights[1], bones=b(1))
    hg, rg, _ = g.render(lp, records=True)
    g.sync()

    def final(i):
        p, given = _morphed(M, weights[i], S, b(i))
        n = motion.vertex_normals_f32(p, S.faces)
        assert not np.array_equal(_bits(n), _bits(given))
        return p, n

    _check_rows(g, S, *final(1))
    _oracle(motion.deformed_description(sd, {S.k: final(1)}), lp, hg, rg, "posed, recomputed")
    c = capi.Scene(sd)
    _set(c, M)
    _attach(c, S)
    c.set_normal_mode(S.k, capi.BF_NORMALS_RECOMPUTE)
    hb, rb, _ = c.render_morph_batch(lp, {M.k: weights}, bones={M.k: btab} if bones else None, transforms=xf, records=True)
    c.sync()
    for i in range(3):
        nodes, rows, normals = c.debug_read_tree(4, i)
        mine, face = _slots(rows, S.k)
        p, n = motion.apply_rigid(*final(i), xf[i, S.k])
        assert np.array_equal(_bits(rows[mine][:, :, :3]), _bits(p[S.faces[face]]))
        assert np.array_equal(_bits(normals[mine][:, :, :3]), _bits(n[S.faces[face]]))
    _oracle(motion.moved_description(motion.deformed_description(sd, {S.k: final(2)}), xf[2]), lp, hb[2], rb[2], "batch version 2, recomputed")


@pytest.mark.parametrize("flag", ["CLASSES", "AOV", "MOMENT", "FAST"])
def test_flags_pass_through(hiplib, flag):
    """A launch flag on a morph batch against the same flag on a deform batch of the numpy-morphed vertices: the records are equal
    bit for bit, so both histograms are fp32 atomic sums of the same addends.  Every addend of these launches is non-negative (range
    mode radiance and its squares under BF_FLAG_MOMENT, the depth AOV) and a cell takes at most N = rays traced addends, so each
    sum lies within gamma_N h / (1 - gamma_N) of the exact one (hist_bound.gamma) and the two within twice that of each other; the
    count channels are equal."""
    sd, lp, S = _range_scene(True)
    M = _targets(S, normal_deltas=True)
    weights, _, xf = _batch_inputs(sd, S, 4)
    lf = _with_flags(lp, getattr(capi, "BF_FLAG_" + flag))
    shape_class = np.arange(len(sd.shapes), dtype=np.uint32) % 2
    shape_class[S.k] = 2

    def scene():
        s = capi.Scene(sd)
        if flag == "CLASSES":
            s.set_classes(shape_class, 3, 0)
        if flag == "AOV":
            s.set_aovs(["depth"])
        return s

    g = scene()
    _set(g, M)
    hs, rs, ss = g.render_morph_batch(lf, {M.k: weights}, transforms=xf, records=True)
    posed = [_morphed(M, weights[i]) for i in range(4)]
    pos = np.ascontiguousarray(np.stack([p for p, _ in posed]))
    nrm = np.ascontiguousarray(np.stack([q for _, q in posed]))
    d = scene()
    hd, rd, sdf = d.render_deform_batch(lf, {M.k: pos}, normals={M.k: nrm}, transforms=xf, records=True)
    assert hs.shape == hd.shape == (4, g.channels(lf)) and hs.any()
    assert ss.kernel_variant == sdf.kernel_variant
    for i in range(4):
        _same(rs[i], rd[i])
    N = int(ss.n_rays_closest + ss.n_rays_shadow)
    gam = hist_bound.gamma(N)
    a, b = hs.astype(np.float64), hd.astype(np.float64)
    assert np.all(a >= 0.0) and np.all(b >= 0.0)
    print(flag, "largest relative difference", float(np.max(np.abs(a - b) / np.maximum(np.maximum(a, b), 1e-300))), "bound", 2.0 * gam / (1.0 - gam))
    assert np.all(np.abs(a - b) <= 2.0 * gam / (1.0 - gam) * np.maximum(a, b))
    if flag == "CLASSES":
        per = hs.reshape(4, 3, -1)
        assert per[:, 2].any() and per[:, 0].any()           # the morphed bar's class and another one both hold returns
        counts = count_channels(lp, sd)
        if len(counts):
            flat_s, flat_d = hs.reshape(4 * 3, -1), hd.reshape(4 * 3, -1)
            assert np.array_equal(flat_s[:, counts], flat_d[:, counts])


def test_morph_sweep_equals_per_pulse_and_deform_sweep(hiplib):
    pytest.importorskip("torch")
    from beifong_amd import sweep
    sd, lp, S = _receive_scene()
    M = _targets(S)
    n = 6
    weights, btab, _ = _batch_inputs(sd, S, n)
    morphs, skins = {M.k: M.dp}, {S.k: (S.index, S.weight)}
    for with_bones in (False, True):
        kw = dict(skins=skins, bones={S.k: btab}) if with_bones else {}
        a = sweep.render_morph_sweep(sd, lp, morphs, {M.k: weights}, n_streams=2, **kw)
        b = sweep.render_morph_sweep(sd, lp, morphs, {M.k: weights}, n_streams=2, per_pulse=True, **kw)
        frames = np.ascontiguousarray(np.stack([_morphed(M, weights[i], S, btab[i] if with_bones else None)[0] for i in range(n)]))
        d = sweep.render_deform_sweep(sd, lp, {M.k: frames}, n_streams=2)
        assert a.shape == b.shape == d.shape == (n, a.shape[1], 3)
        # the count channel is exact; I and Q are fp32 atomic sums of equal addends in another order, held to the oracle below
        assert np.array_equal(a[:, :, 2], b[:, :, 2]) and np.array_equal(a[:, :, 2], d[:, :, 2])
        for i in (1, 4):
            want = motion.deformed_description(sd, {M.k: frames[i]})
            ho, ro, so, add = OracleScene(want).render(lp, records=True, threads=8, addends=True)
            for cube in (a, b, d):
                assert_fp32_sum(cube[i].reshape(-1), add.ref, add.S, add.N, f"sweep pulse {i}", counts=count_channels(lp, want))


def _plate_scene(wavelength=0.1):
    """tests/test_gpu_skin.py's narrow-band front end with a plate facing the radar at x = 5, one target that displaces it along x"""
    sd = SceneDesc()
    lam_nm = wavelength * 1e9
    sd.physics.lambda_min_nm, sd.physics.lambda_max_nm = lam_nm * (1 - 1e-6), lam_nm * (1 + 1e-6)
    c = sd.physics.c
    d0 = T.rotate([1, 0, 0], 90) * T.rotate([0, 1, 0], 90)
    aperture = T.translate([0, 0, 0.3]) * d0 * T.scale([20e-3, 50e-3, 1])
    txa = sd.add_rectangle(aperture, sd.add_diffuse(0.0))
    rxa = sd.add_rectangle(aperture, sd.add_diffuse(0.5))
    sd.add_area_transmitter(txa, 1.0)
    t_total, f_c = 2.0e-7, c / wavelength
    sd.set_receiver(rxa, kind="omnidirectional", adc_sampling_start=0.0, adc_sampling_end=t_total, t_bins=1, f_bins=1,
                    t_bandwidth=t_total, f_bandwidth=2.0 * f_c, freq_centre=f_c, freq_ext=f_c * 2e-6)
    v = np.array([[5.0, -0.5, -0.2], [5.0, 0.5, -0.2], [5.0, 0.5, 0.8], [5.0, -0.5, 0.8]], f32)
    f = np.array([[0, 1, 2], [0, 2, 3]], np.uint32)
    sd.add_mesh(v, f, sd.add_diffuse(0.8, twosided=True))
    sd.finalize()
    lp = capi.make_launch(capi.BF_MODE_RECEIVE_IQ, 1 << 14, seed=4, bins=1, bins_y=1)
    return sd, lp, len(sd.shapes) - 1, v


def test_vibrating_plate_sidebands(hiplib):
    """A plate facing the radar whose single target displaces it along the line of sight, weight a sin(2 pi 4 k / 64) over 64
    pulses: the return of a point at angle theta off the axis is phase-modulated at 4 cycles per sweep with index
    4 pi a cos(theta) / lambda <= 0.8.  Below 0.8 the first Bessel sidebands dominate the higher ones (J1 > 4 J2 there): the
    strongest lines away from zero Doppler are slow-time rows +-4.  No amplitude is asserted."""
    pytest.importorskip("torch")
    from beifong_amd import sweep
    lam, n_pulses, m = 0.1, 64, 4
    sd, lp, k, v = _plate_scene(lam)
    a = 0.8 * lam / (4.0 * np.pi)
    dp = np.ascontiguousarray(np.tile(f32([1.0, 0.0, 0.0]), (1, len(v), 1)))
    weights = np.ascontiguousarray((a * np.sin(2.0 * np.pi * m * np.arange(n_pulses) / n_pulses)).astype(f32)[:, None])
    cube = sweep.render_morph_sweep(sd, lp, {k: dp}, {k: weights}, n_streams=2)
    assert cube.shape == (n_pulses, 1, 3) and np.all(cube[:, 0, 2] == lp.n_paths)
    rd = np.abs(sweep.range_doppler(cube, window=False)[:, 0])
    away = np.argsort(rd[1:])[::-1] + 1                      # non-zero Doppler rows, strongest first
    assert {int(away[0]), int(away[1])} == {m, n_pulses - m}, away[:6]


def _raw_set(lib, g, shape, n_targets, rest, nrm, dp, dn):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return lib.bf_scene_set_morph(g.handle, shape, n_targets, p(rest), p(nrm), p(dp), p(dn))


def test_refusals_leave_the_scene_intact(hiplib):
    lib = hiplib
    sd, lp, S = _range_scene(True)
    M = _targets(S, normal_deltas=True)
    rect = next(i for i, s in enumerate(sd.shapes) if s.type != capi.BF_SHAPE_MESH)
    bus = next(i for i, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH and i != S.k)
    bones = _bend(S, [35.0, -50.0])
    g = capi.Scene(sd)
    _set(g, M)
    _attach(g, S)
    g.pose_morph(M.k, W1, bones=bones)
    h0, r0, _ = g.render(lp, records=True)
    _oracle(_desc(sd, M, W1, S, bones), lp, h0, r0, "before the refusals")
    msg = lambda: lib.bf_last_error().decode()

    def refused(st, *words, status=capi.BF_ERR_INVALID):
        text = msg()
        assert st == status, (st, text)
        for w in words:
            assert w in text, (w, text)
        _same(g.render(lp, records=True)[1], r0)             # a valid render still matches what the oracle confirmed

    def changed(a, at, value):
        b = a.copy()
        b[at] = value
        return b

    ok = (M.rest, M.rest_n, M.dp, M.dn)
    here = "shape %d" % S.k
    refused(_raw_set(lib, g, rect, 5, *ok), "shape %d" % rect)
    refused(_raw_set(lib, g, len(sd.shapes), 5, *ok), "shape %d" % len(sd.shapes))
    refused(_raw_set(lib, g, S.k, 5, None, M.rest_n, M.dp, M.dn), here)
    refused(_raw_set(lib, g, S.k, 5, M.rest, M.rest_n, None, M.dn), here)
    refused(_raw_set(lib, g, S.k, 257, *ok), here, "257")
    refused(_raw_set(lib, g, S.k, 5, changed(M.rest, (7, 1), np.nan), M.rest_n, M.dp, M.dn), here, "vertex 7")
    refused(_raw_set(lib, g, S.k, 5, M.rest, changed(M.rest_n, (9, 0), np.inf), M.dp, M.dn), here, "vertex 9")
    refused(_raw_set(lib, g, S.k, 5, M.rest, M.rest_n, changed(M.dp, (2, 11, 0), np.inf), M.dn), here, "target 2", "vertex 11")
    refused(_raw_set(lib, g, S.k, 5, M.rest, M.rest_n, M.dp, changed(M.dn, (4, 3, 2), np.nan)), here, "target 4", "vertex 3")
    refused(_raw_set(lib, g, S.k, 5, M.rest, None, M.dp, None), here)                                       # the mesh has normals
    busv = _verts(sd, bus)
    busd = np.zeros((5,) + busv.shape, f32)
    refused(_raw_set(lib, g, bus, 5, busv, busv, busd, None), "shape %d" % bus)                              # and this one has none
    refused(_raw_set(lib, g, bus, 5, busv, None, busd, busd), "shape %d" % bus, "normal deltas")            # deltas without rest normals
    # poses
    bp = lambda b: b.ctypes.data_as(C.c_void_p) if b is not None else None
    pose = lambda shape, w, b=None: lib.bf_scene_pose_morph(g.handle, shape, bp(w), bp(b), None)
    refused(pose(bus, W1), "shape %d" % bus, "no morph")
    refused(pose(rect, W1), "shape %d" % rect)
    refused(pose(len(sd.shapes), W1), "shape %d" % len(sd.shapes))
    refused(pose(S.k, None))
    refused(pose(S.k, changed(W1, 3, np.nan)), here, "target 3")
    refused(pose(S.k, W1, changed(bones, (2, 1, 3), np.nan)), here, "bone 2")
    refused(pose(S.k, np.array([3e38, -3e38, 3e38, -3e38, 3e38], f32)), here, "bound")                                                 # no bound that float holds
    assert _raw_set(lib, g, bus, 5, busv, None, busd, None) == capi.BF_OK                                   # a morph, but no skin
    refused(pose(bus, W1, bones), "shape %d" % bus, "no skin")
    # batches
    two = np.ascontiguousarray(np.stack([W1, W2]))
    twob = np.ascontiguousarray(np.stack([bones, _bend(S, [10.0, 10.0])]))
    hist = np.zeros((2, g.channels(lp)), f32)

    def batch(launch, n_renders, shapes, tables, btables=None, xf=None, device=False):
        sh = np.asarray(shapes, np.uint32)
        ptrs = (C.c_void_p * len(tables))(*[t.ctypes.data if t is not None else None for t in tables])
        bptrs = (C.c_void_p * len(btables))(*[t.ctypes.data if t is not None else None for t in btables]) if btables else None
        fn = lib.bf_render_morph_batch_device if device else lib.bf_render_morph_batch
        tail = (None, None, None) if device else (None, None)
        return fn(g.handle, C.byref(launch), n_renders, None, len(shapes), sh.ctypes.data_as(C.c_void_p), ptrs, bptrs,
                  len(sd.shapes) if xf is not None else 0, bp(xf), hist.ctypes.data_as(C.c_void_p), *tail)
    refused(batch(lp, 2, [S.k, S.k], [two, two]), "twice")
    refused(batch(lp, 0, [S.k], [two]), "n_renders")                                                        # the host wrapper's own check
    refused(batch(lp, 0, [S.k], [two], device=True), "n_renders")      # (refused before the histogram pointer is looked at)
    refused(batch(_with_flags(lp, capi.BF_FLAG_ROLLING), 2, [S.k], [two]), "ROLLING")
    film = _launch_like(lp, lp.seed)
    film.spp, film.film_width, film.film_height = 1, 2, 2
    refused(batch(film, 2, [S.k], [two]), "film")
    refused(batch(lp, 2, [rect], [two]), "shape %d" % rect)
    refused(batch(lp, 2, [S.k], [None]), here)
    refused(batch(lp, 2, [S.k], [changed(two, (1, 0), np.inf)]), "render 1", here, "target 0")
    refused(batch(lp, 2, [S.k], [two], [changed(twob, (1, 0, 2, 2), np.inf)]), "render 1", here, "bone 0")
    refused(batch(lp, 2, [bus], [two], [twob]), "shape %d" % bus, "no skin")
    xf = np.ascontiguousarray(np.tile(_identity(sd)[None], (2, 1, 1, 1)).astype(f32))
    xf[1, bus, 0, 0] = 1.5                                   # render 1, the bus: not rigid
    refused(batch(lp, 2, [S.k], [two], None, xf), "render 1", "shape %d" % bus)
    g.sync()
    # removing a morph: a pose is then refused, the mesh stays where it is
    g.set_morph(bus, 0)
    refused(pose(bus, W1), "no morph")
    refused(batch(lp, 2, [bus], [two]), "shape %d" % bus, "no morph")
    # a mesh that carries an emitter: unsupported, named
    e_sd, e_lp, E = _range_scene(False)
    EM = _targets(E)
    e_sd.shapes[E.k].emitter = 0
    e_sd.finalize()
    e = capi.Scene(e_sd)
    _, q0, _ = e.render(e_lp, records=True)
    st = _raw_set(lib, e, E.k, 5, EM.rest, None, EM.dp, None)
    assert st == capi.BF_ERR_UNSUPPORTED and "shape %d" % E.k in msg()
    _same(e.render(e_lp, records=True)[1], q0)
