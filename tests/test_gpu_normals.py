"""Recomputed vertex normals on the device (bf_scene_set_normal_mode, BF_NORMALS_RECOMPUTE): wherever a mesh's base
positions are replaced and the call carries no normals, bf_vertex_normals_kernel computes them from the new positions.  The rows
the device holds are compared bit for bit with tests/normals_ref.py (plain numpy, the oracle's arc cosine), every path bit for bit
with the oracle on motion.deformed_description(sd, {k: (p, normals_ref(p, f))}), histogram cells with tests/hist_bound.py's fp32
summation bound.  No tolerance of its own."""
import collections
import ctypes as C

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, scenes
from beifong_amd.scenedesc import SceneDesc
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.normals_ref import fan, normals_ref
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _launch_like
from tests.test_gpu_deform import deform
from tests.test_gpu_motion import _centre, _identity, _same
from tests.test_gpu_skin import _attach, _bend, _check_rows, _oracle, _posed, _range_scene, _receive_scene, _slots

pytestmark = pytest.mark.gpu
f32 = np.float32
GIVEN, RECOMPUTE = capi.BF_NORMALS_GIVEN, capi.BF_NORMALS_RECOMPUTE
K = 8

Mesh = collections.namedtuple("Mesh", "k faces")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _desc(sd, S, p, xf=None):
    d = motion.deformed_description(sd, {S.k: (p, normals_ref(p, S.faces))})
    return d if xf is None else motion.moved_description(d, xf)


def _others_untouched(before, after, k):
    """rows and normal rows of every shape but k, and the .w words of all of them, bit for bit"""
    (_, r0, n0), (_, r1, n1) = before, after
    other = r0.view(np.uint32)[:, 1, 3] != k
    assert other.any() and (~other).any()
    assert np.array_equal(_bits(r0[other]), _bits(r1[other])) and np.array_equal(_bits(n0[other]), _bits(n1[other]))
    assert np.array_equal(_bits(r0)[:, :, 3], _bits(r1)[:, :, 3]) and np.array_equal(_bits(n0)[:, :, 3], _bits(n1)[:, :, 3])


def _fan_scene():
    """the radar front end, a small rectangle mesh and the 300-fan with its zero-area faces, carrying vertex normals"""
    sd = SceneDesc()
    scenes._radar_frontend(sd)
    mat = sd.add_diffuse(0.5)
    pv, pf = meshgen.rectangle_obj()
    sd.add_mesh(pv + f32(3.0), pf, mat, normals=np.tile(f32([0, 0, 1]), (len(pv), 1)))
    v, f = fan(300, degenerate=True)
    v = np.ascontiguousarray(meshgen.place(v, 75.0, (6.0, -1.5, 0.9)), f32)
    sd.add_mesh(v, f, mat, normals=motion.vertex_normals_f32(v, f))
    sd.finalize()
    return sd, Mesh(len(sd.shapes) - 1, f), v


@pytest.mark.parametrize("kind", ["ripple", "mirror"])
def test_rows_after_an_update(hiplib, kind):
    sd, lp, S = _range_scene(True)
    p, _ = deform(sd, S.k, kind)
    g = capi.Scene(sd)
    before = g.debug_read_tree(4)
    g.set_normal_mode(S.k, RECOMPUTE)
    assert g.normal_mode(S.k) == RECOMPUTE
    _others_untouched(before, g.debug_read_tree(4), S.k)
    _check_rows(g, S, S.rest, S.rest_n)                        # setting the mode changes nothing until the next position update
    g.update_vertices(S.k, p)
    g.sync()
    n = normals_ref(p, S.faces)
    _check_rows(g, S, p, n)
    _others_untouched(before, g.debug_read_tree(4), S.k)
    assert not np.array_equal(_bits(n), _bits(S.rest_n))
    # with a pose on the handle: rigid_apply of the recomputed normals
    xf = _identity(sd)
    xf[S.k] = motion.about(motion.rotation([0, 0, 1], 33.0), _centre(sd, S.k), (0.2, 0.1, 0.0))
    g.transform_meshes(xf)
    _check_rows(g, S, *motion.apply_rigid(p, n, xf[S.k]))
    # ... and an update under that pose
    p2, _ = deform(sd, S.k, "twist")
    g.update_vertices(S.k, p2)
    g.sync()
    _check_rows(g, S, *motion.apply_rigid(p2, normals_ref(p2, S.faces), xf[S.k]))


def test_rows_of_the_fan_and_its_degenerate_faces(hiplib):
    """a vertex of 300 faces (one lane's long loop), zero-area faces among good ones, vertices of zero-area faces only"""
    sd, M, v = _fan_scene()
    g = capi.Scene(sd)
    before = g.debug_read_tree(4)
    g.set_normal_mode(M.k, RECOMPUTE)
    c = v.mean(0)
    p = np.ascontiguousarray(((v - c) * f32([1.2, 0.8, 1.5]) + c + f32(0.03) * np.sin(f32(4.0) * v[:, ::-1])).astype(f32))
    g.update_vertices(M.k, p)
    g.sync()
    n = normals_ref(p, M.faces)
    assert np.array_equal(_bits(n[-2:]), _bits(f32([[1, 0, 0], [1, 0, 0]])))      # named by zero-area faces only
    _check_rows(g, M, p, n)
    _others_untouched(before, g.debug_read_tree(4), M.k)


@pytest.mark.parametrize("kind", ["ripple", "mirror"])
def test_render_after_an_update(hiplib, kind):
    sd, lp, S = _range_scene(True)
    p, _ = deform(sd, S.k, kind)
    g = capi.Scene(sd)
    g.set_normal_mode(S.k, RECOMPUTE)
    g.update_vertices(S.k, p)
    hg, rg, _ = g.render(lp, records=True)
    g.sync()
    _oracle(_desc(sd, S, p), lp, hg, rg, f"recomputed {kind}")
    # the mode matters: a GIVEN handle given the same positions and no normals keeps the rest normals, and renders other paths
    h = capi.Scene(sd)
    h.update_vertices(S.k, p)
    _, rh, _ = h.render(lp, records=True)
    assert not np.array_equal(_bits(rg["L"]), _bits(rh["L"]))


def test_pose_skin(hiplib):
    sd, lp, S = _range_scene(True)
    bones = _bend(S, [35.0, -50.0], root=motion.about(motion.rotation([0, 1, 0], 8.0), S.joints[0], (0.1, -0.05, 0.1)))
    g = capi.Scene(sd)
    _attach(g, S)
    g.set_normal_mode(S.k, RECOMPUTE)
    g.pose_skin(S.k, bones)
    hg, rg, _ = g.render(lp, records=True)
    g.sync()
    p, blended = _posed(S, bones)
    n = normals_ref(p, S.faces)
    _check_rows(g, S, p, n)
    # the blended rest normals are not the normals of the posed surface: at every blended vertex the bits differ
    mixed = S.weight[:, 0] < 1.0
    assert mixed.sum() >= 16
    assert np.all((_bits(n[mixed]) != _bits(blended[mixed])).any(axis=1))
    _oracle(_desc(sd, S, p), lp, hg, rg, "posed, recomputed")


def _frames(sd, S, n=K):
    """n position arrays of the bar (bent by its skin on the host: any [n, nv, 3] would do) and a rigid table per render that
    moves the bar and the bus"""
    pos = np.ascontiguousarray(np.stack([_posed(S, _bend(S, [10.0 * (i + 1), -60.0 + 13.0 * i]))[0] for i in range(n)]))
    xf = np.tile(_identity(sd)[None], (n, 1, 1, 1))
    bus = next(i for i, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH and i != S.k)
    for i in range(n):
        xf[i, bus] = motion.about(motion.rotation([0, 0, 1], 9.0 * (i + 1)), _centre(sd, bus), (0.05 * i, -0.03 * i, 0.0))
        xf[i, S.k] = motion.about(motion.rotation([0, 0, 1], -7.0 * i), _centre(sd, S.k), (0.0, 0.04 * i, 0.0))
    return pos, xf.astype(f32)


@pytest.mark.parametrize("chunk_mb", [None, "1"], ids=["one_chunk", "chunked"])
@pytest.mark.parametrize("what", ["deform", "skin"])
def test_batches(hiplib, monkeypatch, what, chunk_mb):
    """render k of a batch == mode + update / pose + transform_meshes + render on a second handle; one render held to the oracle"""
    sd, lp, S = _range_scene(True)
    pos, xf = _frames(sd, S)
    bones = np.ascontiguousarray(np.stack([_bend(S, [10.0 * (i + 1), -60.0 + 13.0 * i]) for i in range(K)]))
    seeds = [100 + i for i in range(K)]
    g = capi.Scene(sd)
    _attach(g, S)
    g.set_normal_mode(S.k, RECOMPUTE)
    c = g.clone()
    assert c.normal_mode(S.k) == RECOMPUTE
    _, r0, _ = g.render(lp, records=True)
    if chunk_mb:
        monkeypatch.setenv("BF_MOTION_BATCH_MB", chunk_mb)   # below one version: one render per chunk
    if what == "deform":
        hb, rb, sb = g.render_deform_batch(lp, {S.k: pos}, transforms=xf, seeds=seeds, records=True)
    else:
        hb, rb, sb = g.render_skin_batch(lp, {S.k: bones}, transforms=xf, seeds=seeds, records=True)
    if chunk_mb:
        monkeypatch.delenv("BF_MOTION_BATCH_MB")
    assert sb.n_paths == K * lp.n_paths and sb.n_guard == 0
    g.sync()
    ref = capi.Scene(sd)
    _attach(ref, S)
    ref.set_normal_mode(S.k, RECOMPUTE)
    for i in range(K):
        li = _launch_like(lp, seeds[i], flags=lp.flags)
        if what == "deform":
            ref.update_vertices(S.k, pos[i])
        else:
            ref.pose_skin(S.k, bones[i])
        ref.transform_meshes(xf[i])
        _same(rb[i], ref.render(li, records=True)[1])
    i = 5
    li = _launch_like(lp, seeds[i], flags=lp.flags)
    want = _desc(sd, S, pos[i], xf[i])                         # the normals of the UNTRANSFORMED positions, turned by to_world
    ho, ro, so, add = OracleScene(want).render(li, records=True, threads=8, addends=True)
    _same(rb[i], ro)
    assert_fp32_sum(hb[i], add.ref, add.S, add.N, f"{what} batch render {i}", counts=count_channels(li, want))
    if not chunk_mb:
        nodes, rows, normals = g.debug_read_tree(4, version=i)
        mine, face = _slots(rows, S.k)
        _, ni = motion.apply_rigid(pos[i], normals_ref(pos[i], S.faces), xf[i, S.k])
        assert np.array_equal(_bits(normals[mine][:, :, :3]), _bits(ni[S.faces[face]]))
    # the handle and its clone are as they were
    _same(g.render(lp, records=True)[1], r0)
    _same(c.render(lp, records=True)[1], r0)


def test_two_shapes_in_one_batch(hiplib):
    """two recomputing shapes at once; then explicit normals for one of them and none for the other"""
    sd, lp, (S1, S2) = _range_scene(True, second_bar=True)
    n = 2
    p1 = np.ascontiguousarray(np.stack([_posed(S1, _bend(S1, [20.0 * (i + 1), -15.0 * (i + 1)]))[0] for i in range(n)]))
    p2 = np.ascontiguousarray(np.stack([_posed(S2, _bend(S2, [-25.0 * (i + 1)], axis=(0.0, 1.0, 0.2)))[0] for i in range(n)]))
    g = capi.Scene(sd)
    g.set_normal_mode(S1.k, RECOMPUTE)
    g.set_normal_mode(S2.k, RECOMPUTE)
    hb, rb, _ = g.render_deform_batch(lp, {S2.k: p2, S1.k: p1}, records=True)
    g.sync()
    for i in range(n):
        want = motion.deformed_description(sd, {S1.k: (p1[i], normals_ref(p1[i], S1.faces)), S2.k: (p2[i], normals_ref(p2[i], S2.faces))})
        _oracle(want, lp, hb[i], rb[i], f"two recomputing shapes, render {i}")
    # explicit normals win for the call: S2 takes what it is given (deliberately not its surface's), S1 is recomputed
    given = np.ascontiguousarray(np.tile(S2.rest_n[None, ::-1], (n, 1, 1)))
    hb, rb, _ = g.render_deform_batch(lp, {S1.k: p1, S2.k: p2}, normals={S2.k: given}, records=True)
    g.sync()
    i = 1
    want = motion.deformed_description(sd, {S1.k: (p1[i], normals_ref(p1[i], S1.faces)), S2.k: (p2[i], given[i])})
    _oracle(want, lp, hb[i], rb[i], "explicit normals for one shape")


def test_mode_rules(hiplib):
    sd, lp, S = _range_scene(True)
    pa, _ = deform(sd, S.k, "ripple")
    pb, _ = deform(sd, S.k, "twist")
    g = capi.Scene(sd)
    assert g.normal_mode(S.k) == GIVEN
    g.set_normal_mode(S.k, RECOMPUTE)
    # explicit normals win under RECOMPUTE
    mine = np.ascontiguousarray(S.rest_n[::-1])
    g.update_vertices(S.k, pa, mine)
    _check_rows(g, S, pa, mine)
    g.update_vertices(S.k, pa)
    na = normals_ref(pa, S.faces)
    _check_rows(g, S, pa, na)
    # back to GIVEN: a positions-only update keeps the normals last computed
    g.set_normal_mode(S.k, GIVEN)
    g.update_vertices(S.k, pb)
    _check_rows(g, S, pb, na)
    # a clone inherits the mode when it is taken and owns it from then on
    g.set_normal_mode(S.k, RECOMPUTE)
    c = g.clone()
    assert c.normal_mode(S.k) == RECOMPUTE
    c.set_normal_mode(S.k, GIVEN)
    assert g.normal_mode(S.k) == RECOMPUTE and c.normal_mode(S.k) == GIVEN
    # copy on write between clones: the source's update does not show in the clone, nor the clone's in the source
    g.update_vertices(S.k, pa)
    _check_rows(g, S, pa, na)
    _check_rows(c, S, pb, na)
    c.set_normal_mode(S.k, RECOMPUTE)
    c.update_vertices(S.k, pb)
    nb = normals_ref(pb, S.faces)
    _check_rows(c, S, pb, nb)
    _check_rows(g, S, pa, na)
    # a rebuild between two updates: the index is per vertex and face, not per slot, and no record changes
    _, r_a, _ = g.render(lp, records=True)
    g.rebuild_bvh()
    _same(g.render(lp, records=True)[1], r_a)
    g.update_vertices(S.k, pb)
    hg, rg, _ = g.render(lp, records=True)
    g.sync()
    _check_rows(g, S, pb, nb)
    _same(rg, c.render(lp, records=True)[1])
    _oracle(_desc(sd, S, pb), lp, hg, rg, "update after a rebuild")


def test_device_form(hiplib):
    torch = pytest.importorskip("torch")
    sd, lp, S = _range_scene(True)
    p, _ = deform(sd, S.k, "twist")
    g = capi.Scene(sd)
    g.set_normal_mode(S.k, RECOMPUTE)
    stream = torch.cuda.Stream()
    dv = torch.from_numpy(p).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g.update_vertices_device(S.k, dv.data_ptr(), None, float(np.abs(p).max()), stream=stream.cuda_stream)
    g.sync()                                                 # clean: nothing beyond the bound, every normal finite
    hg, rg, _ = g.render(lp, records=True)
    _check_rows(g, S, p, normals_ref(p, S.faces))
    _oracle(_desc(sd, S, p), lp, hg, rg, "device form, recomputed")


def test_refusals_leave_the_scene_intact(hiplib):
    sd, lp, S = _range_scene(True)
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    rect = next(i for i, s in enumerate(sd.shapes) if s.type != capi.BF_SHAPE_MESH)
    plain = next(i for i, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH and not s.normals)
    lib = hiplib
    mode = C.c_uint32(9)
    for shape, m, text in [(len(sd.shapes), RECOMPUTE, "shape %d" % len(sd.shapes)), (rect, RECOMPUTE, "not a mesh"), (S.k, 2, "unknown mode"),
                           (plain, RECOMPUTE, "without vertex normals")]:
        assert lib.bf_scene_set_normal_mode(g.handle, shape, m) == capi.BF_ERR_INVALID, (shape, m)
        assert text in lib.bf_last_error().decode(), lib.bf_last_error()
    for shape in (len(sd.shapes), rect):
        assert lib.bf_scene_get_normal_mode(g.handle, shape, C.byref(mode)) == capi.BF_ERR_INVALID
    assert lib.bf_scene_get_normal_mode(g.handle, S.k, None) == capi.BF_ERR_INVALID and mode.value == 9
    assert g.normal_mode(S.k) == GIVEN and g.normal_mode(plain) == GIVEN
    _same(g.render(lp, records=True)[1], r0)
    # a mesh that carries an emitter: unsupported, as a vertex update of it
    sd2, lp2, S2 = _range_scene(True)
    sd2.shapes[S2.k].emitter = 0
    sd2.finalize()
    g2 = capi.Scene(sd2)
    _, q0, _ = g2.render(lp2, records=True)
    with pytest.raises(capi.BeifongError) as e:
        g2.set_normal_mode(S2.k, RECOMPUTE)
    assert "status %d" % capi.BF_ERR_UNSUPPORTED in str(e.value) and "shape %d" % S2.k in str(e.value)
    _same(g2.render(lp2, records=True)[1], q0)


def test_deform_sweep_equals_per_pulse(hiplib):
    pytest.importorskip("torch")
    from beifong_amd import sweep
    sd, lp, S = _receive_scene()
    nrm = motion.vertex_normals_f32(S.rest, S.faces)
    sd.shapes[S.k].normals = nrm.ctypes.data_as(C.POINTER(C.c_float))
    sd._keep.append(nrm)
    sd.finalize()
    n = 6
    pos = np.ascontiguousarray(np.stack([_posed(S, _bend(S, [12.0 * (i + 1), -9.0 * (i + 1)]))[0] for i in range(n)]))
    a = sweep.render_deform_sweep(sd, lp, {S.k: pos}, n_streams=2, recompute_normals=(S.k,))
    b = sweep.render_deform_sweep(sd, lp, {S.k: pos}, n_streams=2, per_pulse=True, recompute_normals=(S.k,))
    assert a.shape == b.shape and np.all(a[:, :, 2].sum(1) == b[:, :, 2].sum(1))
    i = 4
    want = _desc(sd, S, pos[i])
    ho, ro, so, add = OracleScene(want).render(lp, records=True, threads=8, addends=True)
    for cube in (a, b):
        assert_fp32_sum(cube[i].reshape(-1), add.ref, add.S, add.N, f"sweep pulse {i}", counts=count_channels(lp, want))


def test_mitsuba_layer_recomputes_on_the_cached_handle(hiplib, tmp_path):
    """parameters_changed(recompute_normals=True) on a rendered scene: no handle is created, no normals are uploaded, and the normal
    rows the device computed equal the host mesh's rewritten buffer bit for bit"""
    from beifong_amd import mitsuba as m
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_gpu_host import RADAR_MESH_SCENE, _write_ply_be
    m.set_variant("scalar_rgb")
    v, f = meshgen.bus(600, seed=1)
    v = np.ascontiguousarray(meshgen.place(v, -20.0, (12.0, 3.0, 1.7)), f32)
    f = np.asarray(f, np.uint32)
    _write_ply_be(tmp_path / "a.ply", v, f, normals=meshgen.vertex_normals(v, f))
    scene = load_string(RADAR_MESH_SCENE % ("ply", "a.ply", ""), base_dir=str(tmp_path))
    sensor = scene.sensors()[0]
    scene.integrator().render(scene, sensor)
    assert scene.device_creations() == 1
    mesh = scene.shapes()[2]
    c = v.mean(0)
    v2 = np.ascontiguousarray(((v - c) * f32([1.0, 0.8, 1.3]) + c + f32(0.05) * np.sin(f32(7.0) * v[:, ::-1])).astype(f32))
    mesh.set_vertex_positions(v2)
    mesh.parameters_changed(recompute_normals=True)
    assert scene.device_creations() == 1
    host_n = mesh.vertex_normals_buffer().reshape(-1, 3)
    assert np.array_equal(_bits(host_n), _bits(normals_ref(v2, f)))
    g = capi.Scene.borrow(_host.lib().bfh_scene_device(scene._ptr, sensor._ptr), owner=scene)
    assert g.normal_mode(2) == RECOMPUTE
    _check_rows(g, Mesh(2, f), v2, host_n)
    scene.integrator().render(scene, sensor)
    assert scene.device_creations() == 1
