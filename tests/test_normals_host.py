"""Recomputed vertex normals (bf_vertex_normals, BF_NORMALS_RECOMPUTE), the parts that need no GPU: the host entry
is the fp32 statement bit for bit (tests/normals_ref.py: plain numpy, the oracle's arc cosine), the statement is the float64
angle-weighted normal to a few ulp, the summation order is part of it, bad arguments are refused, and the mitsuba-shaped layer
rewrites a host mesh's normal buffer with it."""
import ctypes as C

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion
from tests.normals_ref import fan, normals_ref

f32 = np.float32
PLACE = (75.0, (6.0, -1.5, 0.9))         # as the GPU scenes place the bar
# |fp32 statement - float64 statement| per component.  The statement's own error on these meshes is below 2^-23 (measured; each
# normal is a sum of at most eight terms of magnitude < pi, normalised); the float64 side adds half an ulp of its final cast
# to float32 (2^-25 below 1), and the margin of 4 covers that and the cases where both roundings pull apart.
TOL64 = 4 * 2.0 ** -23


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _placed(v):
    return np.ascontiguousarray(meshgen.place(v, *PLACE), f32)


def _bar():
    v, f, _, _ = meshgen.jointed_bar(3, 8, 6, radius=0.4)
    return _placed(v), f


def _bus(n):
    v, f = meshgen.bus(n, seed=1)
    return _placed(v), np.asarray(f, np.uint32)


MESHES = {
    "bar": _bar,
    "bus600": lambda: _bus(600),
    "bus5000": lambda: _bus(5000),
    "fan300": lambda: (lambda v, f: (_placed(v), f))(*fan(300)),
    "degenerate": lambda: (lambda v, f: (_placed(v), f))(*fan(12, degenerate=True)),
}


def _valence(nv, f):
    return np.bincount(np.asarray(f).reshape(-1), minlength=nv)


@pytest.mark.parametrize("name", list(MESHES))
def test_host_entry_is_the_statement_bit_for_bit(name):
    v, f = MESHES[name]()
    got = motion.vertex_normals_f32(v, f)
    assert got.dtype == f32 and got.shape == v.shape
    assert np.array_equal(_bits(got), _bits(normals_ref(v, f)))
    assert np.array_equal(_bits(got), _bits(capi.vertex_normals(v, f)))
    unused = _valence(len(v), f) == 0
    if name.startswith("bus"):
        assert unused.sum() == 12                              # vertices no face names
    assert np.array_equal(_bits(got[unused]), _bits(np.tile(f32([1, 0, 0]), (int(unused.sum()), 1))))
    if name == "fan300":
        assert _valence(len(v), f)[0] == 300
    if name == "degenerate":
        nv = len(v)
        d, e, e2 = nv - 3, nv - 2, nv - 1
        # named by zero-area faces only: (1, 0, 0); the zero-area face (0, 1, d) adds nothing to its three vertices
        assert np.array_equal(_bits(got[[e, e2]]), _bits(f32([[1, 0, 0], [1, 0, 0]])))
        keep = np.ones(len(f), bool)
        keep[[12, 14, 15]] = False                             # the three zero-area faces (fan(12): faces 0..11 are the fan's)
        without = normals_ref(v, f[keep])
        assert np.array_equal(_bits(got[:nv - 2]), _bits(without[:nv - 2]))
        assert not np.array_equal(got[d], f32([1, 0, 0]))      # d has the good face (d, 3, 2)


@pytest.mark.parametrize("name", ["bar", "bus600", "bus5000"])
def test_statement_against_float64(name):
    v, f = MESHES[name]()
    got = motion.vertex_normals_f32(v, f).astype(np.float64)
    ref = meshgen.vertex_normals(v, f).astype(np.float64)
    used = _valence(len(v), f) > 0
    err = np.abs(got[used] - ref[used]).max()
    print(f"{name}: max |fp32 statement - float64| = {err / 2.0 ** -23:.3f} x 2^-23 over {int(used.sum())} vertices")
    assert err <= TOL64
    assert np.array_equal(got[~used], ref[~used]) and np.all(got[~used] == [1.0, 0.0, 0.0])


def test_the_order_of_the_sum_is_part_of_the_statement():
    v, f = MESHES["bus600"]()
    base = motion.vertex_normals_f32(v, f)
    # a permutation that keeps every vertex's incident faces in their relative order: faces are moved only past faces they
    # share no vertex with (adjacent transpositions of vertex-disjoint neighbours, many of them)
    g = f.copy()
    rng = np.random.default_rng(7)
    moved = 0
    for _ in range(20000):
        i = int(rng.integers(0, len(g) - 1))
        if not set(g[i]) & set(g[i + 1]):
            g[[i, i + 1]] = g[[i + 1, i]]
            moved += 1
    assert moved > 1000 and not np.array_equal(g, f)
    assert np.array_equal(_bits(motion.vertex_normals_f32(v, g)), _bits(base))
    # reversed: every vertex sums its faces backwards.  Last bits may move; the float64 statement does not care
    rev = motion.vertex_normals_f32(v, f[::-1].copy())
    assert np.array_equal(_bits(rev), _bits(normals_ref(v, f[::-1])))
    used = _valence(len(v), f) > 0
    ref = meshgen.vertex_normals(v, f).astype(np.float64)
    assert np.abs(rev.astype(np.float64)[used] - ref[used]).max() <= TOL64
    n_diff = int((_bits(rev) != _bits(base)).any(axis=1).sum())
    print(f"reversed face order: {n_diff} of {int(used.sum())} normals differ in bits")
    assert n_diff > 0                                          # fp32 addition is not associative: the order is observable


def test_bad_arguments_are_refused():
    lib = capi.load_library()
    v, f = MESHES["bar"]()
    out = np.zeros_like(v)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.bf_vertex_normals(len(v), None, len(f), vp(f), vp(out)) == capi.BF_ERR_INVALID
    assert b"bf_vertex_normals" in lib.bf_last_error() and b"null" in lib.bf_last_error()
    assert lib.bf_vertex_normals(len(v), vp(v), len(f), None, vp(out)) == capi.BF_ERR_INVALID
    assert lib.bf_vertex_normals(len(v), vp(v), len(f), vp(f), None) == capi.BF_ERR_INVALID
    bad = f.copy()
    bad[17, 2] = len(v)
    assert lib.bf_vertex_normals(len(v), vp(v), len(bad), vp(bad), vp(out)) == capi.BF_ERR_INVALID
    msg = lib.bf_last_error()
    assert b"face 17" in msg and str(len(v)).encode() in msg
    assert not out.any()                                       # a refused call writes nothing
    with pytest.raises(capi.BeifongError, match="face 17"):
        capi.vertex_normals(v, bad)
    with pytest.raises(TypeError):
        capi.vertex_normals(v.astype(np.float64), f)
    with pytest.raises(TypeError):
        capi.vertex_normals(v, f.astype(np.int64))
    with pytest.raises(ValueError):
        capi.vertex_normals(v, f[:, :2])
    # nothing to do is not an error
    assert lib.bf_vertex_normals(0, None, 0, None, None) == capi.BF_OK
    assert np.array_equal(capi.vertex_normals(v, np.zeros((0, 3), np.uint32)), np.tile(f32([1, 0, 0]), (len(v), 1)))


def test_mitsuba_layer_rewrites_the_host_normals(tmp_path):
    """parameters_changed(recompute_normals=True) with nothing cached: the host mesh's normal buffer becomes the statement of its
    positions, bit for bit; the default call leaves it alone; a mesh without normals is refused."""
    from beifong_amd import mitsuba as m
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_gpu_host import RADAR_MESH_SCENE, _write_ply_be
    m.set_variant("scalar_rgb")
    v, f = meshgen.bus(400, seed=1)
    v = np.ascontiguousarray(v, f32)
    f = np.asarray(f, np.uint32)
    _write_ply_be(tmp_path / "n.ply", v, f, normals=meshgen.vertex_normals(v, f))
    _write_ply_be(tmp_path / "p.ply", v, f)
    scene = load_string(RADAR_MESH_SCENE % ("ply", "n.ply", ""), base_dir=str(tmp_path))
    mesh = scene.shapes()[2]
    n0 = mesh.vertex_normals_buffer()
    assert n0.size == v.size
    v2 = (v * f32([1.0, 1.3, 0.8]) + f32(0.05) * np.sin(f32(3.0) * v[:, ::-1])).astype(f32)
    mesh.set_vertex_positions(v2)
    mesh.parameters_changed()                                  # the default: the normal buffer is left alone
    assert np.array_equal(_bits(mesh.vertex_normals_buffer()), _bits(n0))
    mesh.parameters_changed(recompute_normals=True)
    assert scene.device_creations() == 0
    want = normals_ref(v2, f)
    assert np.array_equal(_bits(mesh.vertex_normals_buffer()), _bits(want.reshape(-1)))
    assert not np.array_equal(_bits(want.reshape(-1)), _bits(n0))
    # a later flatten reads the new buffer
    sh = scene.flat_desc(scene.sensors()[0]).desc.shapes[2]
    assert np.array_equal(_bits(np.ctypeslib.as_array(sh.normals, shape=(sh.n_vertices, 3))), _bits(want))
    # a mesh without vertex normals: refused, as the reference throws (face normals: the loader computes none)
    plain = load_string(RADAR_MESH_SCENE % ("ply", "p.ply", '<boolean name="face_normals" value="true"/>'), base_dir=str(tmp_path))
    with pytest.raises(_host.HostError, match="no vertex normals"):
        plain.shapes()[2].parameters_changed(recompute_normals=True)
    with pytest.raises(_host.HostError):
        plain.shapes()[1].parameters_changed(recompute_normals=True)      # a rectangle
