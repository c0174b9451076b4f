"""Skinned meshes (bf_scene_set_skin, bf_scene_pose_skin, bf_render_skin_batch): the device computes the vertices of
a mesh from a rest pose, four bone slots per vertex and a few 3x4 matrices, then treats them as a vertex update.  Every path is
held bit for bit to the oracle on motion.deformed_description(motion.apply_skin(...)), the numpy statement of the arithmetic;
histogram cells to tests/hist_bound.py's fp32 summation bound.  No tolerance of its own, except where two fp32 atomic sums of the
same addends are compared with each other (test_flags_pass_through states its bound)."""
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

pytestmark = pytest.mark.gpu
f32 = np.float32
N_PATHS = 1 << 13

Skin = collections.namedtuple("Skin", "k rest rest_n faces index weight joints n_bones")


def _bar(n_bones=3, n_around=8, n_along=6, radius=0.4):
    """jointed_bar and its joints (n_bones + 1 points on the axis: the ends and the joints between the bones)"""
    v, f, index, weight = meshgen.jointed_bar(n_bones, n_around, n_along, radius=radius)
    joints = np.stack([np.arange(n_bones + 1, dtype=np.float64), np.zeros(n_bones + 1), np.zeros(n_bones + 1)], -1)
    return v, f, index, weight, joints


def _skin_of(sd, k, f, index, weight, joints, normals):
    rest = _verts(sd, k)
    rest_n = np.ctypeslib.as_array(sd.shapes[k].normals, shape=(sd.shapes[k].n_vertices, 3)).copy() if normals else None
    return Skin(k, rest, rest_n, f, index, weight, joints, int(index.max()) + 1)


def _range_scene(normals, n_bones=3, second_bar=False):
    """the radar front end, ground and a small bus of tests/test_gpu_motion.py's scenes, with a jointed bar (304 triangles) as the
    skinned mesh; second_bar: another one with two bones"""
    sd = SceneDesc()
    scenes._radar_frontend(sd)
    scenes._ground(sd)
    mat = sd.add_roughconductor(alpha=0.1, twosided=True, specular_reflectance=1.0)
    v, f = meshgen.bus(600, seed=1)
    sd.add_mesh(meshgen.place(v, -20.0, (12.0, 3.0, 1.7)), f, mat)
    bars = []
    for nb, yaw, at in [(n_bones, 75.0, (6.0, -1.5, 0.9))] + ([(2, -60.0, (4.5, 2.0, 0.7))] if second_bar else []):
        bv, bf, index, weight, joints = _bar(nb)
        pv = meshgen.place(bv, yaw, at)
        sd.add_mesh(pv, bf, mat, normals=meshgen.vertex_normals(pv, bf) if normals else None)
        bars.append((len(sd.shapes) - 1, bf, index, weight, meshgen.place(joints, yaw, at).astype(np.float64)))
    sd.finalize()
    lp = capi.make_launch(capi.BF_MODE_RANGE, N_PATHS, seed=3, bins=1024, bin_width=0.03)
    skins = [_skin_of(sd, k, bf, index, weight, joints, normals) for k, bf, index, weight, joints in bars]
    return (sd, lp, skins) if second_bar else (sd, lp, skins[0])


def _receive_scene():
    """scenes.bus_receive with the bar in the bus's place: 2.5 times the size and turned broadside to the radar before the builder
    places it (yaw -20 degrees, at (10, 3, 1.7))"""
    bv, bf, index, weight, joints = _bar(3)
    local = lambda a: meshgen.place(np.asarray(a, np.float64) - [1.5, 0.0, 0.0], 90.0, (0.0, 0.0, 0.0), 2.5)
    sd, lp = scenes.bus_receive(n_paths=N_PATHS, mesh=(local(bv), bf))
    lp.mode = capi.BF_MODE_RECEIVE_IQ
    k = next(i for i, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH)
    return sd, lp, _skin_of(sd, k, bf, index, weight, meshgen.place(local(joints), -20.0, (10.0, 3.0, 1.7)).astype(np.float64), False)


def _m4(m):
    out = np.eye(4)
    out[:3] = np.asarray(m, np.float64).reshape(3, 4)
    return out


def _bend(S, angles, axis=(0.2, 0.1, 1.0), root=None):
    """float32[n_bones, 3, 4]: bone 0 = `root` (identity), bone k = bone k - 1 after a turn by angles[k - 1] degrees about joint k"""
    m = np.eye(4) if root is None else _m4(root)
    bones = [m[:3].copy()]
    for k in range(1, S.n_bones):
        m = m @ _m4(motion.about(motion.rotation(axis, angles[k - 1]), S.joints[k]))
        bones.append(m[:3].copy())
    return np.ascontiguousarray(np.stack(bones), f32)


def _attach(g, S):
    g.set_skin(S.k, S.n_bones, S.rest, S.index, S.weight, rest_normals=S.rest_n)


def _posed(S, bones):
    return motion.apply_skin(S.rest, S.rest_n, S.index, S.weight, bones)


def _posed_desc(sd, S, bones, xf=None):
    d = motion.deformed_description(sd, {S.k: _posed(S, bones)})
    return d if xf is None else motion.moved_description(d, xf)


def _oracle(sd_new, lp, hg, rg, what):
    ho, ro, so, add = OracleScene(sd_new).render(lp, records=True, threads=8, addends=True)
    _same(rg, ro)
    if hg is not None:
        assert_fp32_sum(hg, add.ref, add.S, add.N, what, counts=count_channels(lp, sd_new))
    return ro


@pytest.mark.parametrize("case", ["range", "range_normals", "receive_iq"])
def test_pose_then_render(hiplib, case):
    sd, lp, S = _receive_scene() if case == "receive_iq" else _range_scene(case == "range_normals")
    bones = _bend(S, [35.0, -50.0], root=motion.about(motion.rotation([0, 1, 0], 8.0), S.joints[0], (0.1, -0.05, 0.1)))
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    _attach(g, S)
    _same(g.render(lp, records=True)[1], r0)                 # attaching a skin moves nothing
    g.pose_skin(S.k, bones)
    hg, rg, _ = g.render(lp, records=True)
    g.sync()
    assert not np.array_equal(rg["L"], r0["L"])              # the pose shows
    # every joint is bent: a blended vertex is neither bone's image of its rest position
    p, _ = _posed(S, bones)
    mixed = (S.weight[:, 0] < 1.0)
    assert mixed.sum() >= 16
    for slot in (0, 1):
        for v in np.nonzero(mixed)[0][:8]:
            assert not np.array_equal(p[v], motion.apply_rigid(S.rest[v:v + 1], None, bones[S.index[v, slot]])[0][0])
    _oracle(_posed_desc(sd, S, bones), lp, hg, rg, f"{case} posed")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _slots(rows, k):
    w = rows.view(np.uint32)
    mine = np.nonzero(w[:, 1, 3] == k)[0]
    return mine, w[mine, 0, 3] - w[mine, 0, 3].min()


def _check_rows(g, S, p, n):
    """the triangle rows (and vertex normals) of shape S.k as the device holds them: the posed vertices, float for float"""
    nodes, rows, normals = g.debug_read_tree(4)
    mine, face = _slots(rows, S.k)
    assert len(mine) == len(S.faces)
    want = p[S.faces[face]]                                  # [slots, 3 corners, 3]
    assert np.array_equal(_bits(rows[mine][:, :, :3]), _bits(want))
    if n is not None:
        assert np.array_equal(_bits(normals[mine][:, :, :3]), _bits(n[S.faces[face]]))


@pytest.mark.parametrize("normals", [False, True], ids=["plain", "normals"])
def test_what_the_device_wrote(hiplib, normals):
    sd, lp, S = _range_scene(normals)
    bones = _bend(S, [-25.0, 60.0])
    g = capi.Scene(sd)
    before = check_scene(g)
    _attach(g, S)
    g.pose_skin(S.k, bones)
    g.sync()                                                 # no violation: the bound the library computed held
    p, n = _posed(S, bones)
    _check_rows(g, S, p, n)
    check_scene(g, before)                                   # both trees bound the rows they hold
    # under a pose of the handle: rigid_apply of the skinned vertices
    xf = _identity(sd)
    xf[S.k] = motion.about(motion.rotation([0, 0, 1], 33.0), _centre(sd, S.k), (0.2, 0.1, 0.0))
    g.transform_meshes(xf)
    g.sync()
    _check_rows(g, S, *motion.apply_rigid(p, n, xf[S.k]))
    check_scene(g, before)
    assert float(g.debug_origin_scale()) < 100.0


def _strip(nv, rng):
    """a mesh of nv vertices in [-1, 1]^3: a triangle strip (one degenerate triangle for fewer than three vertices)"""
    v = np.ascontiguousarray(rng.uniform(-1.0, 1.0, (nv, 3)), f32)
    f = np.array([[i, i + 1, i + 2] for i in range(nv - 2)] or [[0, nv - 1, 0]], np.uint32)
    return v, f


def _rigid_bones(n, rng):
    return np.ascontiguousarray(np.stack([motion.about(motion.rotation(rng.normal(size=3), rng.uniform(-90, 90)), rng.uniform(-1, 1, 3),
                                                       rng.uniform(-0.5, 0.5, 3)) for _ in range(n)]), f32)


def _weights(nv, rng):
    w = rng.random((nv, 4)) + 0.05
    return np.ascontiguousarray(w / w.sum(1, keepdims=True), f32)


EDGE = ["nv1", "nv63", "nv257", "nv1000", "one_bone", "bones256", "same_bone", "zero_weight_large_bone", "affine"]


@pytest.mark.parametrize("case", EDGE)
def test_kernel_edge_shapes(hiplib, case):
    """the grid's ragged end, one block and several, the smallest and the largest bone table, and what a lane may hold in its four
    slots; the device's rows against numpy's, bit for bit"""
    rng = np.random.default_rng(EDGE.index(case) + 1)
    nv = {"nv1": 1, "nv63": 63, "nv257": 257, "nv1000": 1000, "bones256": 1000}.get(case, 300)
    n_bones = {"one_bone": 1, "bones256": 256, "zero_weight_large_bone": 4}.get(case, 3)
    with_normals = case in ("nv257", "bones256", "affine")
    v, f = _strip(nv, rng)
    nrm = np.ascontiguousarray(rng.normal(size=(nv, 3)), f32) if with_normals else None
    index = rng.integers(0, n_bones, (nv, 4)).astype(np.uint32)
    weight = _weights(nv, rng)
    bones = _rigid_bones(n_bones, rng)
    if case == "same_bone":
        index[:] = index[:, :1]
    elif case == "zero_weight_large_bone":
        index[:, :2] = rng.integers(0, 3, (nv, 2))
        index[:, 2:] = 3
        weight[:, 2:] = 0.0
        weight[:, 1] = f32(1.0) - weight[:, 0]
        bones[3] = 1e30                                      # large but finite: fl(0 q) = 0 whatever q is, as long as q is finite
    elif case == "affine":
        bones[1, :, :3] = (bones[1, :, :3].astype(np.float64) @ np.diag([1.5, 0.7, 1.2])).astype(f32)      # non-uniform scale
        bones[2, :, :3] = np.array([[1.0, 0.4, 0.0], [0.0, 1.0, -0.3], [0.2, 0.0, 0.8]], f32)               # a shear
    sd = SceneDesc()
    scenes._radar_frontend(sd)
    mat = sd.add_diffuse(0.5)
    pv, pf = meshgen.rectangle_obj()
    sd.add_mesh(pv + f32(3.0), pf, mat)
    sd.add_mesh(v, f, mat, normals=nrm)
    sd.finalize()
    k = len(sd.shapes) - 1
    S = Skin(k, v, nrm, f, index, weight, None, n_bones)
    g = capi.Scene(sd)
    before = check_scene(g)
    _attach(g, S)
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
    g2 = capi.Scene(sd)
    _attach(g2, S)
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


def test_pose_ordering_and_updates(hiplib):
    """pose then transform and the reverse; update_vertices after a pose replaces the base, a pose after it starts from the skin's
    rest arrays again; a pose after a rebuild"""
    sd, lp, S = _range_scene(True)
    bones, bones2 = _bend(S, [40.0, -30.0]), _bend(S, [-20.0, 55.0], axis=(1.0, 0.0, 0.3))
    xf = _identity(sd)
    xf[S.k] = motion.about(motion.rotation([0, 0, 1], 50.0), _centre(sd, S.k), (0.3, 0.4, 0.0))
    a = capi.Scene(sd)
    _attach(a, S)
    a.pose_skin(S.k, bones)
    a.transform_meshes(xf)
    ha, ra, _ = a.render(lp, records=True)
    _oracle(_posed_desc(sd, S, bones, xf), lp, ha, ra, "pose, transform")
    b = capi.Scene(sd)
    _attach(b, S)
    b.transform_meshes(xf)
    b.pose_skin(S.k, bones)
    _same(b.render(lp, records=True)[1], ra)
    # a vertex update after a pose: the base is what the update gives
    moved = (S.rest + f32(0.25)).astype(f32)
    b.update_vertices(S.k, moved, S.rest_n)
    hb, rb, _ = b.render(lp, records=True)
    _oracle(motion.moved_description(motion.deformed_description(sd, {S.k: (moved, S.rest_n)}), xf), lp, hb, rb, "update after a pose")
    # ... and a pose after it starts from the skin's rest arrays, not from the updated base
    b.pose_skin(S.k, bones2)
    hb, rb, _ = b.render(lp, records=True)
    ro2 = _oracle(_posed_desc(sd, S, bones2, xf), lp, hb, rb, "pose after an update")
    # a rebuild keeps the skin valid
    a.rebuild_bvh()
    _same(a.render(lp, records=True)[1], ra)
    a.pose_skin(S.k, bones2)
    _same(a.render(lp, records=True)[1], ro2)
    check_scene(a)
    a.sync()
    b.sync()


def test_clones_copy_on_write(hiplib):
    sd, lp, S = _range_scene(False)
    ba, bb = _bend(S, [30.0, 30.0]), _bend(S, [-45.0, 20.0])
    g = capi.Scene(sd)
    _attach(g, S)
    c = g.clone()                                            # shares the skin
    _, r0, _ = g.render(lp, records=True)
    c.pose_skin(S.k, ba)
    hc, rc, _ = c.render(lp, records=True)
    _same(g.render(lp, records=True)[1], r0)                 # the original is untouched
    ra = _oracle(_posed_desc(sd, S, ba), lp, hc, rc, "clone posed")
    g.pose_skin(S.k, bb)
    _same(c.render(lp, records=True)[1], ra)                 # and the reverse
    hg, rg, _ = g.render(lp, records=True)
    rb = _oracle(_posed_desc(sd, S, bb), lp, hg, rg, "original posed")
    # a new skin on the clone alone: the original keeps the one it has
    one = Skin(S.k, S.rest, None, S.faces, np.zeros_like(S.index), np.tile(np.array([1, 0, 0, 0], f32), (len(S.rest), 1)), S.joints, 1)
    _attach(c, one)
    lone = np.ascontiguousarray(motion.rigid(t=(0.0, 0.5, 0.2))[None], f32)
    c.pose_skin(S.k, lone)
    hc, rc, _ = c.render(lp, records=True)
    _oracle(_posed_desc(sd, one, lone), lp, hc, rc, "clone with its own skin")
    g.pose_skin(S.k, ba)
    _same(g.render(lp, records=True)[1], ra)
    g.close()
    _same(c.render(lp, records=True)[1], rc)
    assert not np.array_equal(rb["L"], ra["L"])


def test_rolling_sequence_around_a_pose(hiplib):
    pytest.importorskip("torch")
    sd, lp, S = _range_scene(False)
    bones = _bend(S, [35.0, -50.0])
    g = capi.Scene(sd)
    _attach(g, S)
    seeds = [21, 22, 23, 24]
    seq = _Sequence(g, lp, seeds)
    seq.issue([0, 1])
    g.pose_skin(S.k, bones)                                  # finishes the open sequence first
    seq.issue([2, 3])
    g.flush()
    h, recs = seq.results()
    new_sd = _posed_desc(sd, S, bones)
    old, new = OracleScene(sd), OracleScene(new_sd)
    for i, seed in enumerate(seeds):
        li = _launch_like(lp, seed)
        ho, ro, so, add = (old if i < 2 else new).render(li, records=True, threads=8, addends=True)
        _same(recs[i], ro)
        assert_fp32_sum(h[i], add.ref, add.S, add.N, f"rolling render {i}", counts=count_channels(li, sd if i < 2 else new_sd))


K = 8


def _batch_inputs(sd, S, n=K):
    """n poses that bend both joints differently, and a rigid table per render that moves the bar and the bus"""
    bones = np.ascontiguousarray(np.stack([_bend(S, [10.0 * (i + 1), -60.0 + 13.0 * i], root=motion.rigid(t=(0.02 * i, 0.0, 0.01 * i)))
                                           for i in range(n)]))
    xf = np.tile(_identity(sd)[None], (n, 1, 1, 1))
    bus = next(i for i, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH and i != S.k)
    for i in range(n):
        xf[i, bus] = motion.about(motion.rotation([0, 0, 1], 9.0 * (i + 1)), _centre(sd, bus), (0.05 * i, -0.03 * i, 0.0))
        xf[i, S.k] = motion.about(motion.rotation([0, 0, 1], -7.0 * i), _centre(sd, S.k), (0.0, 0.04 * i, 0.0))
    return bones, xf.astype(f32)


@pytest.mark.parametrize("chunk_mb", [None, "1"], ids=["one_chunk", "chunked"])
def test_batch_equals_pose_transform_render(hiplib, monkeypatch, chunk_mb):
    sd, lp, S = _range_scene(True)
    bones, xf = _batch_inputs(sd, S)
    seeds = [100 + i for i in range(K)]
    g = capi.Scene(sd)
    _attach(g, S)
    c = g.clone()
    _, r0, _ = g.render(lp, records=True)
    if chunk_mb:
        monkeypatch.setenv("BF_MOTION_BATCH_MB", chunk_mb)   # below one version: one render per chunk
    hb, rb, sb = g.render_skin_batch(lp, {S.k: bones}, transforms=xf, seeds=seeds, records=True)
    if chunk_mb:
        monkeypatch.delenv("BF_MOTION_BATCH_MB")
    assert sb.n_paths == K * lp.n_paths and sb.n_guard == 0
    g.sync()
    ref = capi.Scene(sd)
    _attach(ref, S)
    for i in range(K):
        li = _launch_like(lp, seeds[i], flags=lp.flags)
        ref.pose_skin(S.k, bones[i])
        ref.transform_meshes(xf[i])
        _same(rb[i], ref.render(li, records=True)[1])
    for i in (0, 5):
        li = _launch_like(lp, seeds[i], flags=lp.flags)
        want = _posed_desc(sd, S, bones[i], xf[i])
        ho, ro, so, add = OracleScene(want).render(li, records=True, threads=8, addends=True)
        _same(rb[i], ro)
        assert_fp32_sum(hb[i], add.ref, add.S, add.N, f"skin batch render {i}", counts=count_channels(li, want))
    # the handle and its clone are as they were
    _same(g.render(lp, records=True)[1], r0)
    _same(c.render(lp, records=True)[1], r0)


def test_two_skinned_shapes_in_one_batch(hiplib):
    sd, lp, (S1, S2) = _range_scene(False, second_bar=True)
    n = 3
    b1 = np.ascontiguousarray(np.stack([_bend(S1, [20.0 * (i + 1), -15.0 * (i + 1)]) for i in range(n)]))
    b2 = np.ascontiguousarray(np.stack([_bend(S2, [-25.0 * (i + 1)], axis=(0.0, 1.0, 0.2)) for i in range(n)]))
    g = capi.Scene(sd)
    _attach(g, S1)
    _attach(g, S2)
    hb, rb, _ = g.render_skin_batch(lp, {S2.k: b2, S1.k: b1}, records=True)
    g.sync()
    for i in range(n):
        want = motion.deformed_description(sd, {S1.k: _posed(S1, b1[i])[0], S2.k: _posed(S2, b2[i])[0]})
        _oracle(want, lp, hb[i], rb[i], f"two skins, render {i}")
    # one of the two alone: the other stays at the handle's base
    _, r1, _ = g.render_skin_batch(lp, {S2.k: b2[:1]}, records=True)
    _oracle(motion.deformed_description(sd, {S2.k: _posed(S2, b2[0])[0]}), lp, None, r1[0], "one of two")


def test_skin_sweep_equals_per_pulse(hiplib):
    pytest.importorskip("torch")
    from beifong_amd import sweep
    sd, lp, S = _receive_scene()
    n = 6
    bones = np.ascontiguousarray(np.stack([_bend(S, [12.0 * (i + 1), -9.0 * (i + 1)]) for i in range(n)]))
    skins = {S.k: (S.index, S.weight)}
    a = sweep.render_skin_sweep(sd, lp, skins, {S.k: bones}, n_streams=2)
    b = sweep.render_skin_sweep(sd, lp, skins, {S.k: bones}, n_streams=2, per_pulse=True)
    assert a.shape == b.shape and np.all(a[:, :, 2].sum(1) == b[:, :, 2].sum(1))
    i = 4
    want = _posed_desc(sd, S, bones[i])
    ho, ro, so, add = OracleScene(want).render(lp, records=True, threads=8, addends=True)
    for cube in (a, b):
        assert_fp32_sum(cube[i].reshape(-1), add.ref, add.S, add.N, f"sweep pulse {i}", counts=count_channels(lp, want))


def test_flags_pass_through(hiplib):
    """BF_FLAG_CLASSES on a skin batch against the same flag on a deform batch of the host-skinned vertices: the records are equal
    bit for bit, so both histograms are fp32 atomic sums of the same addends.  Range-mode addends are non-negative and a cell takes
    at most N = rays traced addends, so each sum lies within gamma_N h / (1 - gamma_N) of the exact one (hist_bound.gamma) and
    the two within twice that of each other; the count channels are equal."""
    sd, lp, S = _range_scene(True)
    bones, xf = _batch_inputs(sd, S, 4)
    lc = _with_flags(lp, capi.BF_FLAG_CLASSES)
    shape_class = np.arange(len(sd.shapes), dtype=np.uint32) % 2
    shape_class[S.k] = 2
    g = capi.Scene(sd)
    g.set_classes(shape_class, 3, 0)
    _attach(g, S)
    hs, rs, ss = g.render_skin_batch(lc, {S.k: bones}, transforms=xf, records=True)
    posed = [_posed(S, bones[i]) for i in range(4)]
    pos = np.ascontiguousarray(np.stack([p for p, _ in posed]))
    nrm = np.ascontiguousarray(np.stack([q for _, q in posed]))
    d = capi.Scene(sd)
    d.set_classes(shape_class, 3, 0)
    hd, rd, sdf = d.render_deform_batch(lc, {S.k: pos}, normals={S.k: nrm}, transforms=xf, records=True)
    assert hs.shape == hd.shape == (4, 3 * g.channels(lp))
    for i in range(4):
        _same(rs[i], rd[i])
    N = int(ss.n_rays_closest + ss.n_rays_shadow)
    gam = hist_bound.gamma(N)
    a, b = hs.astype(np.float64), hd.astype(np.float64)
    assert np.all(a >= 0.0) and np.all(b >= 0.0)
    assert np.all(np.abs(a - b) <= 2.0 * gam / (1.0 - gam) * np.maximum(a, b))
    per = hs.reshape(4, 3, -1)
    assert per[:, 2].any() and per[:, 0].any()               # the skinned bar's class and another one both hold returns
    counts = count_channels(lp, sd)
    if len(counts):
        flat_s, flat_d = hs.reshape(4 * 3, -1), hd.reshape(4 * 3, -1)
        assert np.array_equal(flat_s[:, counts], flat_d[:, counts])


def _raw_set(lib, g, shape, n_bones, rest, nrm, index, weight):
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
    return lib.bf_scene_set_skin(g.handle, shape, n_bones, p(rest), p(nrm), p(index), p(weight))


def test_refusals_leave_the_scene_intact(hiplib):
    lib = hiplib
    sd, lp, S = _range_scene(True)
    plain_sd, _, P = _range_scene(False)
    rect = next(i for i, s in enumerate(sd.shapes) if s.type != capi.BF_SHAPE_MESH)
    bus = next(i for i, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH and i != S.k)
    bones = _bend(S, [35.0, -50.0])
    g = capi.Scene(sd)
    _attach(g, S)
    g.pose_skin(S.k, bones)
    h0, r0, _ = g.render(lp, records=True)
    _oracle(_posed_desc(sd, S, bones), lp, h0, r0, "before the refusals")
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

    ok = (S.rest, S.rest_n, S.index, S.weight)
    refused(_raw_set(lib, g, rect, 3, *ok), "shape %d" % rect)
    refused(_raw_set(lib, g, len(sd.shapes), 3, *ok), "shape %d" % len(sd.shapes))
    refused(_raw_set(lib, g, S.k, 3, None, S.rest_n, S.index, S.weight), "shape %d" % S.k)
    refused(_raw_set(lib, g, S.k, 3, S.rest, S.rest_n, None, S.weight), "shape %d" % S.k)
    refused(_raw_set(lib, g, S.k, 3, S.rest, S.rest_n, S.index, None), "shape %d" % S.k)
    refused(_raw_set(lib, g, S.k, 3, changed(S.rest, (7, 1), np.nan), S.rest_n, S.index, S.weight), "vertex 7")
    refused(_raw_set(lib, g, S.k, 3, S.rest, changed(S.rest_n, (9, 0), np.inf), S.index, S.weight), "vertex 9")
    refused(_raw_set(lib, g, S.k, 3, S.rest, S.rest_n, S.index, changed(S.weight, (5, 2), np.nan)), "vertex 5")
    refused(_raw_set(lib, g, S.k, 3, S.rest, S.rest_n, changed(S.index, (11, 3), 3), S.weight), "vertex 11", "bone 3")
    refused(_raw_set(lib, g, S.k, 3, S.rest, S.rest_n, S.index, changed(changed(S.weight, (4, 2), -0.25), (4, 3), 0.25)), "vertex 4")
    refused(_raw_set(lib, g, S.k, 3, S.rest, S.rest_n, S.index, changed(S.weight, (6, 3), 2e-3)), "vertex 6")
    refused(_raw_set(lib, g, S.k, 257, *ok), "257")
    refused(_raw_set(lib, g, S.k, 3, S.rest, None, S.index, S.weight), "shape %d" % S.k)                    # the mesh has normals
    refused(_raw_set(lib, g, bus, 3, _verts(sd, bus), _verts(sd, bus), S.index, S.weight), "shape %d" % bus)      # and this one has none
    # poses
    bp = lambda b: b.ctypes.data_as(C.c_void_p) if b is not None else None
    refused(lib.bf_scene_pose_skin(g.handle, bus, bp(bones), None), "shape %d" % bus, "no skin")
    refused(lib.bf_scene_pose_skin(g.handle, rect, bp(bones), None), "shape %d" % rect)
    refused(lib.bf_scene_pose_skin(g.handle, len(sd.shapes), bp(bones), None), "shape %d" % len(sd.shapes))
    refused(lib.bf_scene_pose_skin(g.handle, S.k, None, None))
    refused(lib.bf_scene_pose_skin(g.handle, S.k, bp(changed(bones, (2, 1, 3), np.nan)), None), "bone 2")
    refused(lib.bf_scene_pose_skin(g.handle, S.k, bp(changed(bones, (1, 0, 0), 3e38)), None), "bound")     # no finite bound
    # batches
    two = np.ascontiguousarray(np.stack([bones, _bend(S, [10.0, 10.0])]))
    hist = np.zeros((2, g.channels(lp)), f32)

    def batch(launch, n_renders, shapes, tables, xf=None):
        sh = np.asarray(shapes, np.uint32)
        ptrs = (C.c_void_p * len(tables))(*[t.ctypes.data if t is not None else None for t in tables])
        return lib.bf_render_skin_batch(g.handle, C.byref(launch), n_renders, None, len(shapes), sh.ctypes.data_as(C.c_void_p), ptrs,
                                        len(sd.shapes) if xf is not None else 0, bp(xf), hist.ctypes.data_as(C.c_void_p), None, None)
    refused(batch(lp, 2, [S.k, S.k], [two, two]), "twice")
    refused(batch(lp, 0, [S.k], [two]))
    refused(batch(_with_flags(lp, capi.BF_FLAG_ROLLING), 2, [S.k], [two]), "ROLLING")
    film = _launch_like(lp, lp.seed)
    film.spp, film.film_width, film.film_height = 1, 2, 2
    refused(batch(film, 2, [S.k], [two]), "film")
    refused(batch(lp, 2, [bus], [two]), "shape %d" % bus, "no skin")
    refused(batch(lp, 2, [rect], [two]), "shape %d" % rect)
    refused(batch(lp, 2, [S.k], [None]), "shape %d" % S.k)
    refused(batch(lp, 2, [S.k], [changed(two, (1, 0, 2, 2), np.inf)]), "render 1", "bone 0")
    xf = np.ascontiguousarray(np.tile(_identity(sd)[None], (2, 1, 1, 1)).astype(f32))
    xf[1, bus, 0, 0] = 1.5                                   # render 1, the bus: not rigid
    refused(batch(lp, 2, [S.k], [two], xf), "render 1", "shape %d" % bus)
    g.sync()
    # removing the skin: a pose is then refused, the mesh stays where it is
    g.set_skin(S.k, 0)
    refused(lib.bf_scene_pose_skin(g.handle, S.k, bp(bones), None), "no skin")
    # a mesh that carries an emitter: unsupported, named
    e_sd, e_lp, E = _range_scene(False)
    e_sd.shapes[E.k].emitter = 0
    e_sd.finalize()
    e = capi.Scene(e_sd)
    _, q0, _ = e.render(e_lp, records=True)
    st = _raw_set(lib, e, E.k, 3, E.rest, None, E.index, E.weight)
    assert st == capi.BF_ERR_UNSUPPORTED and "shape %d" % E.k in msg()
    _same(e.render(e_lp, records=True)[1], q0)
    del plain_sd, P


def _swing_scene(wavelength=0.1):
    """scenes.plate_doppler's narrow-band front end with a two-bone bar across the line of sight instead of the plate: the bar
    lies along y at x = 5, joint on the axis of the radar"""
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
    bv, bf, index, weight, joints = _bar(2, 8, 6, radius=0.25)
    pv = meshgen.place(bv, 90.0, (5.0, -1.0, 0.3))           # x -> y: the bar spans y in [-1, 1]
    sd.add_mesh(pv, bf, sd.add_diffuse(0.8, twosided=True))
    sd.finalize()
    lp = capi.make_launch(capi.BF_MODE_RECEIVE_IQ, 1 << 14, seed=4, bins=1, bins_y=1)
    k = len(sd.shapes) - 1
    return sd, lp, _skin_of(sd, k, bf, index, weight, meshgen.place(joints, 90.0, (5.0, -1.0, 0.3)).astype(np.float64), False)


def test_swinging_bone_sidebands(hiplib):
    """A two-bone bar across the line of sight whose outer bone swings about the vertical axis through the joint by
    theta_k = theta_0 sin(2 pi k / 16) over 64 pulses: a point of the outer bone at distance r from the joint moves along the
    line of sight by r theta, so its return is phase-modulated at 4 cycles per sweep with index 4 pi r theta_0 / lambda <= 0.8 at
    the tip (r = 1).  Below 0.8 the first Bessel sidebands dominate the higher ones for every r (J1 > 4 J2 there), and the inner
    bone only adds to zero Doppler: the strongest lines away from zero Doppler are slow-time bins +-4."""
    pytest.importorskip("torch")
    from beifong_amd import sweep
    lam, n_pulses = 0.1, 64
    sd, lp, S = _swing_scene(lam)
    theta0 = np.degrees(0.8 * lam / (4.0 * np.pi * 1.0))
    bones = np.ascontiguousarray(np.stack([_bend(S, [theta0 * np.sin(2.0 * np.pi * i / 16.0)], axis=(0.0, 0.0, 1.0)) for i in range(n_pulses)]))
    cube = sweep.render_skin_sweep(sd, lp, {S.k: (S.index, S.weight)}, {S.k: bones}, n_streams=2)
    assert cube.shape == (n_pulses, 1, 3) and np.all(cube[:, 0, 2] == lp.n_paths)
    rd = np.abs(sweep.range_doppler(cube, window=False)[:, 0])
    away = np.argsort(rd[1:])[::-1] + 1                      # non-zero Doppler bins, strongest first
    assert {int(away[0]), int(away[1])} == {4, n_pulses - 4}, away[:6]
    assert max(rd[8], rd[n_pulses - 8]) < min(rd[4], rd[n_pulses - 4]) and rd[0] > rd[4]
