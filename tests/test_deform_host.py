"""Vertex updates (bf_scene_update_vertices), the parts that need no GPU: the ABI stays what it was, the four new
entry points exist, the Python layer refuses malformed arrays before it touches the library, and motion.deformed_description
builds the scene a bf_scene_create would have to rebuild."""
import ctypes as C
import os

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion
from beifong_amd.scenedesc import SceneDesc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["bf_scene_update_vertices", "bf_scene_update_vertices_device", "bf_render_deform_batch_device", "bf_render_deform_batch"]


@pytest.fixture(scope="module")
def mitsuba():
    from beifong_amd import mitsuba as m
    m.set_variant("scalar_rgb")
    return m


def test_symbols_exported_and_declared():
    lib = capi.load_library()
    header = open(os.path.join(ROOT, "include", "beifong_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), name
        assert f"bf_status {name}(" in header, name
        assert name in capi.EXPORTED_SYMBOLS


def test_abi_unchanged():
    lib = capi.load_library()
    assert capi.BF_ABI_VERSION == 5 and lib.bf_version() == 5
    assert "#define BF_ABI_VERSION 5" in open(os.path.join(ROOT, "include", "beifong_hip.h")).read()
    # the sizes recorded from the library before vertex updates existed (BF_ABI_MATERIAL .. BF_ABI_BATCH): no struct grew or moved
    recorded = [44, 248, 208, 416, 480, 80, 16, 192, 72, 24]
    assert [lib.bf_abi_sizeof(i) for i in range(len(recorded))] == recorded
    assert [C.sizeof(t) for t in capi.ABI_STRUCTS] == recorded
    assert lib.bf_abi_sizeof(len(recorded)) == 0


def _two_meshes():
    sd = SceneDesc()
    mat = sd.add_diffuse(0.5)
    v, f = meshgen.bus(400, seed=1)
    sd.add_mesh(v, f, mat)
    v2, f2, _ = meshgen.car_body(600, seed=2, with_normals=True)
    sd.add_mesh(v2, f2, mat, normals=meshgen.vertex_normals(v2, f2))
    return sd


class _NoLibrary:
    """stands in for the loaded library: any call through it fails the test"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) before the arguments were checked")


def _dry_scene(sd):
    s = capi.Scene.__new__(capi.Scene)
    s.lib, s.holder, s.handle, s._borrowed = _NoLibrary(), sd, C.c_void_p(1), True
    return s


def test_capi_refuses_before_the_library():
    sd = _two_meshes()
    g = _dry_scene(sd)
    nv = sd.shapes[0].n_vertices
    good = np.zeros((nv, 3), np.float32)
    with pytest.raises(TypeError):
        g.update_vertices(0, good.astype(np.float64))
    with pytest.raises(ValueError):
        g.update_vertices(0, good[:-1])
    with pytest.raises(ValueError):
        g.update_vertices(0, np.zeros((nv, 2), np.float32))
    with pytest.raises(ValueError):
        g.update_vertices(0, good, normals=np.zeros((nv - 1, 3), np.float32))
    with pytest.raises(TypeError):
        g.update_vertices(0, good, normals=np.zeros((nv, 3), np.float64))
    with pytest.raises(ValueError):
        g.update_vertices(-1, good)
    lp = capi.make_launch(capi.BF_MODE_RANGE, 16, seed=1, bins=8, bin_width=1.0)
    k3 = np.zeros((3, nv, 3), np.float32)
    with pytest.raises(ValueError):
        g.render_deform_batch(lp, [(0, k3), (0, k3)])                         # a shape listed twice
    with pytest.raises(ValueError):
        g.render_deform_batch(lp, {0: k3[0]})                                 # no render axis
    with pytest.raises(TypeError):
        g.render_deform_batch(lp, {0: k3.astype(np.float64)})
    with pytest.raises(ValueError):
        g.render_deform_batch(lp, {0: k3, 1: np.zeros((2, sd.shapes[1].n_vertices, 3), np.float32)})      # 3 slices and 2
    with pytest.raises(ValueError):
        g.render_deform_batch(lp, {0: k3[:, :-1]})
    with pytest.raises(ValueError):
        g.render_deform_batch(lp, {0: k3}, normals={1: k3})                   # normals for a shape without positions
    with pytest.raises(ValueError):
        g.render_deform_batch(lp, {0: k3}, seeds=[1, 2])
    with pytest.raises(ValueError):
        g.render_deform_batch_device(lp, 3, dict([(0, 4096)]), 4096, 1.0, seeds=[1])


def _arr(ptr, n, w):
    return np.ctypeslib.as_array(ptr, shape=(n, w))


def test_deformed_description():
    sd = _two_meshes().finalize()
    s0, s1 = sd.shapes[0], sd.shapes[1]
    p1 = (_arr(s1.positions, s1.n_vertices, 3) * np.float32(1.25)).astype(np.float32)
    n1 = meshgen.vertex_normals(p1, _arr(s1.indices, s1.n_faces, 3)).astype(np.float32)
    out = motion.deformed_description(sd, {1: (p1, n1)})
    assert len(out.shapes) == len(sd.shapes)
    o0, o1 = out.shapes[0], out.shapes[1]
    # exactly the arrays named: shape 0 is untouched, shape 1 has new positions and normals and everything else of its own
    assert C.addressof(o0.positions.contents) == C.addressof(s0.positions.contents)
    assert np.array_equal(_arr(o1.positions, o1.n_vertices, 3).view(np.uint32), p1.view(np.uint32))
    assert np.array_equal(_arr(o1.normals, o1.n_vertices, 3).view(np.uint32), n1.view(np.uint32))
    assert C.addressof(o1.indices.contents) == C.addressof(s1.indices.contents)
    assert (o1.n_vertices, o1.n_faces, o1.material, o1.emitter, o1.type) == (s1.n_vertices, s1.n_faces, s1.material, s1.emitter, s1.type)
    assert bool(o1.texcoords) == bool(s1.texcoords)
    assert bytes(out.sensor) == bytes(sd.sensor) and bytes(out.physics) == bytes(sd.physics)
    assert len(out.materials) == len(sd.materials) and len(out.emitters) == len(sd.emitters)
    # positions alone: the normals stay the mesh's own
    only = motion.deformed_description(sd, {1: p1})
    assert C.addressof(only.shapes[1].normals.contents) == C.addressof(s1.normals.contents)
    # composes with moved_description: deform, then move == apply_rigid of the new arrays
    xf = np.tile(motion.rigid(), (len(sd.shapes), 1, 1))
    xf[1] = motion.about(motion.rotation([0, 0, 1], 30.0), [1.0, 2.0, 0.0], (0.5, 0.0, 0.1))
    both = motion.moved_description(out, xf)
    pm, nm = motion.apply_rigid(p1, n1, xf[1])
    assert np.array_equal(_arr(both.shapes[1].positions, s1.n_vertices, 3).view(np.uint32), pm.view(np.uint32))
    assert np.array_equal(_arr(both.shapes[1].normals, s1.n_vertices, 3).view(np.uint32), nm.view(np.uint32))
    assert C.addressof(both.shapes[0].positions.contents) == C.addressof(s0.positions.contents)
    with pytest.raises(ValueError):
        motion.deformed_description(sd, {0: (p1[: s0.n_vertices], n1[: s0.n_vertices])})      # shape 0 has no normals
    with pytest.raises(ValueError):
        motion.deformed_description(sd, {0: p1[:5]})
    with pytest.raises(TypeError):
        motion.deformed_description(sd, {1: p1.astype(np.float64)})
    with pytest.raises(ValueError):
        motion.deformed_description(sd, {7: p1})


def test_mitsuba_layer_vertex_buffers_on_the_host(mitsuba, tmp_path):
    """Shape.vertex_positions_buffer / set_vertex_positions on the host mesh (no device scene yet: nothing is created), and the
    refusals: a shape that is not a mesh, a wrong size, a wrong dtype, a non-finite value, normals on a mesh without them."""
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_gpu_host import RADAR_MESH_SCENE, _write_ply_be
    v, f = meshgen.bus(400, seed=1)
    v = np.ascontiguousarray(v, np.float32)
    _write_ply_be(tmp_path / "m.ply", v, f)
    scene = load_string(RADAR_MESH_SCENE % ("ply", "m.ply", '<boolean name="face_normals" value="true"/>'), base_dir=str(tmp_path))
    rect, mesh = scene.shapes()[1], scene.shapes()[2]
    assert np.array_equal(mesh.vertex_positions_buffer().view(np.uint32), v.reshape(-1).view(np.uint32))
    assert mesh.vertex_normals_buffer().size == 0
    v2 = (v * np.float32(1.5)).astype(np.float32)
    mesh.set_vertex_positions(v2)
    mesh.parameters_changed()                                # no cached handle: nothing to update, nothing created
    assert scene.device_creations() == 0
    assert np.array_equal(mesh.vertex_positions_buffer().view(np.uint32), v2.reshape(-1).view(np.uint32))
    sh = scene.flat_desc(scene.sensors()[0]).desc.shapes[2]
    assert np.array_equal(np.ctypeslib.as_array(sh.positions, shape=(sh.n_vertices, 3)).view(np.uint32), v2.view(np.uint32))
    for call in (rect.vertex_positions_buffer, rect.vertex_normals_buffer, lambda: rect.set_vertex_positions(v2), rect.parameters_changed,
                 lambda: mesh.set_vertex_positions(v2[:-1]), lambda: mesh.set_vertex_normals(v2)):
        with pytest.raises(_host.HostError):
            call()
    bad = v2.copy()
    bad[3, 1] = np.inf
    with pytest.raises(_host.HostError):
        mesh.set_vertex_positions(bad)
    with pytest.raises(TypeError):
        mesh.set_vertex_positions(v2.astype(np.float64))
    assert np.array_equal(mesh.vertex_positions_buffer().view(np.uint32), v2.reshape(-1).view(np.uint32))      # refusals wrote nothing
