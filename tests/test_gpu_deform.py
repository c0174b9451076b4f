"""Per-vertex mesh updates (bf_scene_update_vertices): the base vertices of a mesh are replaced on the device, the
BVHs re-fitted, and every path renders bit-identically to a scene created from the new vertices (motion.deformed_description):
closest hits do not depend on the tree, and a triangle row is a plain copy of three vertices.

Tolerances: none of its own.  Exact mode is held to the oracle on the rebuilt description (records bit for bit, histogram cells
within tests/hist_bound.py's fp32 summation bound); BF_FLAG_FAST to a freshly created GPU scene (equal records and ray counts)."""
import ctypes as C

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, scenes
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _launch_like
from tests.test_gpu_motion import _identity, _meshes, _multi_mesh, _poses, _receive_iq, _same, _with_flags

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def mitsuba():
    from beifong_amd import mitsuba as m
    m.set_variant("scalar_rgb")
    return m


def _verts(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()


def _faces(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.indices, shape=(s.n_faces, 3)).copy()


def _has_normals(sd, k):
    return bool(sd.shapes[k].normals)


def _target(sd):
    """the mesh the tests deform: the one with vertex normals if there is one, else the first"""
    ms = _meshes(sd)
    return next((k for k in ms if _has_normals(sd, k)), ms[0])


def deform(sd, k, kind):
    """(positions, normals or None) float32 of mesh k deformed: 'ripple' a small displacement a sin(kappa . p) along the
    normal; 'twist' a non-uniform scale by 1.5 / 0.7 / 1.2 about the centre plus a twist about z growing with height;
    'mirror' x -> 2 c_x - x, which flips every winding."""
    p = _verts(sd, k).astype(np.float64)
    f = _faces(sd, k)
    c = 0.5 * (p.min(0) + p.max(0))
    if kind == "ripple":
        n = meshgen.vertex_normals(p.astype(f32), f).astype(np.float64)
        q = p + 0.02 * np.sin(p @ np.array([9.0, 5.0, 13.0]))[:, None] * n
    elif kind == "twist":
        d = (p - c) * np.array([1.5, 0.7, 1.2])
        ang = 1.1 * (p[:, 2] - p[:, 2].min())
        cs, sn = np.cos(ang), np.sin(ang)
        q = np.stack([cs * d[:, 0] - sn * d[:, 1], sn * d[:, 0] + cs * d[:, 1], d[:, 2]], 1) + c
    elif kind == "mirror":
        q = p.copy()
        q[:, 0] = 2.0 * c[0] - p[:, 0]
    else:
        raise ValueError(kind)
    q = np.ascontiguousarray(q, dtype=f32)
    nrm = np.ascontiguousarray(meshgen.vertex_normals(q, f), dtype=f32) if _has_normals(sd, k) else None
    return q, nrm


def _oracle_check(sd_new, lp, hg, rg, what):
    ho, ro, so, add = OracleScene(sd_new).render(lp, records=True, threads=8, addends=True)
    _same(rg, ro)
    assert_fp32_sum(hg, add.ref, add.S, add.N, what, counts=count_channels(lp, sd_new))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("kind", ["ripple", "twist", "mirror"])
@pytest.mark.parametrize("case", ["range", "range_normals", "receive_iq"])
def test_update_equals_rebuilt_scene(hiplib, case, kind, fast):
    sd, lp = _receive_iq() if case == "receive_iq" else _multi_mesh(case == "range_normals")
    lp = _with_flags(lp, capi.BF_FLAG_FAST if fast else 0)
    k = _target(sd)
    v, n = deform(sd, k, kind)
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    g.update_vertices(k, v, n)
    hg, rg, sg = g.render(lp, records=True)
    fresh_sd = motion.deformed_description(sd, {k: (v, n)})
    assert not np.array_equal(rg["L"], r0["L"])              # the deformation shows
    if fast:
        hf, rf, sf = capi.Scene(fresh_sd).render(lp, records=True)
        _same(rg, rf)
        assert sg.n_rays_closest == sf.n_rays_closest and sg.n_rays_shadow == sf.n_rays_shadow
    else:
        _oracle_check(fresh_sd, lp, hg, rg, f"{case} {kind}")


def test_update_composes_with_the_pose(hiplib):
    """update then transform, transform then update: both are create-with-V + transform.  translate after an update; batch
    mesh offsets on top; positions alone keep the normals the mesh has."""
    sd, lp = _multi_mesh(True)
    k = _target(sd)
    v, n = deform(sd, k, "twist")
    xf = _poses(sd)
    new_sd = motion.deformed_description(sd, {k: (v, n)})
    want_sd = motion.moved_description(new_sd, xf)
    a = capi.Scene(sd)
    a.update_vertices(k, v, n)
    a.transform_meshes(xf)
    ha, ra, _ = a.render(lp, records=True)
    _oracle_check(want_sd, lp, ha, ra, "update, transform")
    b = capi.Scene(sd)
    b.transform_meshes(xf)
    b.update_vertices(k, v, n)
    hb, rb, _ = b.render(lp, records=True)
    _same(rb, ra)                                            # (histograms are atomic sums: held to the oracle above, not to each other)
    # translate after an update: every mesh at fl(base + o), the updated one from its new base, normals as given
    off = [0.3, -0.2, 0.05]
    a.translate_meshes(off)
    ht, rt, _ = a.render(lp, records=True)
    xo = _identity(sd)
    for m in _meshes(sd):
        xo[m] = motion.rigid(t=off)
    _oracle_check(motion.moved_description(new_sd, xo), lp, ht, rt, "update, translate")
    ref = capi.Scene(new_sd)
    ref.translate_meshes(off)
    _same(rt, ref.render(lp, records=True)[1])
    # an update under a translation
    c = capi.Scene(sd)
    c.translate_meshes(off)
    c.update_vertices(k, v, n)
    _same(c.render(lp, records=True)[1], rt)
    # positions alone
    d = capi.Scene(sd)
    d.update_vertices(k, v)
    hd, rd, _ = d.render(lp, records=True)
    _oracle_check(motion.deformed_description(sd, {k: v}), lp, hd, rd, "positions alone")


def test_batch_offsets_on_top_of_an_update(hiplib):
    sd, lp = _receive_iq()
    k = _target(sd)
    v, n = deform(sd, k, "ripple")
    g = capi.Scene(sd)
    g.update_vertices(k, v, n)
    offs = np.array([[0.0, 0.0, 0.0], [0.25, -0.1, 0.0], [-0.5, 0.3, 0.02]], f32)
    _, rb, _ = g.render_batch(lp, len(offs), offsets=offs, records=True)
    new_sd = motion.deformed_description(sd, {k: (v, n)})
    ref = capi.Scene(new_sd)
    _, rr, _ = ref.render_batch(lp, len(offs), offsets=offs, records=True)
    for i in range(len(offs)):
        _same(rb[i], rr[i])
    _, r0, _ = g.render(lp, records=True)
    ho, ro, _ = OracleScene(new_sd).render(lp, records=True, threads=8)
    _same(rb[0], ro)
    _same(r0, ro)


def test_update_by_an_offset_is_a_translation(hiplib):
    """fl(p0 + o) computed in numpy and given as new vertices == bf_scene_translate_meshes(o): the newest path and the oldest"""
    sd, lp = _receive_iq()
    off = np.array([0.3, -0.2, 0.05], f32)
    g = capi.Scene(sd)
    for k in _meshes(sd):
        g.update_vertices(k, (_verts(sd, k) + off[None, :]).astype(f32))
    hg, rg, sg = g.render(lp, records=True)
    t = capi.Scene(sd)
    t.translate_meshes(off)
    ht, rt, st = t.render(lp, records=True)
    _same(rg, rt)
    assert sg.n_rays_closest == st.n_rays_closest and sg.n_rays_shadow == st.n_rays_shadow


def test_ray_intersect_matches_rebuilt_scene(hiplib):
    sd, _ = _multi_mesh(True)
    k = _target(sd)
    v, n = deform(sd, k, "twist")
    g = capi.Scene(sd)
    g.update_vertices(k, v, n)
    rng = np.random.default_rng(11)
    cnt = 4096
    tgt = v[_faces(sd, k)[rng.integers(0, sd.shapes[k].n_faces, cnt)]].astype(np.float64).mean(1)      # centroids of its faces
    o = np.where(np.arange(cnt)[:, None] % 2 == 0, np.array([0.0, 0.0, 0.3]), tgt + rng.normal(size=(cnt, 3)) * 5.0)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((cnt, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 0.0, d, np.inf
    a = g.ray_intersect(rays)
    b = capi.Scene(motion.deformed_description(sd, {k: (v, n)})).ray_intersect(rays)
    assert np.array_equal(a["raw"].view(np.uint32), b["raw"].view(np.uint32))          # every SurfaceInteraction field
    assert np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["shape"], b["shape"])
    # aimed at the deformed mesh: the half of the rays that start at the radar sees it unoccluded
    assert np.isfinite(a["t"]).sum() > cnt // 2 and (a["shape"][np.isfinite(a["t"])] == k).sum() > cnt // 4


@pytest.mark.parametrize("knob", [{"BF_NO_WIDE_BVH": "1"}, {"BF_QUANT_BVH": "1"}, {"megakernel": "1"}], ids=["no_wide", "quant", "megakernel"])
def test_tree_variants(hiplib, monkeypatch, knob):
    mega = "megakernel" in knob
    for name, val in ({} if mega else knob).items():
        monkeypatch.setenv(name, val)
    for sd, lp in (_multi_mesh(True), _receive_iq()):
        if mega:
            lp = _with_flags(lp, capi.BF_FLAG_MEGAKERNEL)
        k = _target(sd)
        v, n = deform(sd, k, "twist")
        g = capi.Scene(sd)
        if "BF_QUANT_BVH" in knob:
            assert g.info().trace_node_bytes == 64
        g.update_vertices(k, v, n)
        _, rg, _ = g.render(lp, records=True)
        _, ro, _ = OracleScene(motion.deformed_description(sd, {k: (v, n)})).render(lp, records=True, threads=8)
        _same(rg, ro)


def test_clones_copy_on_write(hiplib):
    sd, lp = _multi_mesh(True)
    k = _target(sd)
    va, na = deform(sd, k, "ripple")
    vb, nb = deform(sd, k, "mirror")
    g = capi.Scene(sd)
    c = g.clone()
    _, r0, _ = g.render(lp, records=True)
    c.update_vertices(k, va, na)
    _, rc, _ = c.render(lp, records=True)
    _same(g.render(lp, records=True)[1], r0)                 # the parent is untouched
    _, ra, _ = OracleScene(motion.deformed_description(sd, {k: (va, na)})).render(lp, records=True, threads=8)
    _same(rc, ra)
    g.update_vertices(k, vb, nb)
    _same(c.render(lp, records=True)[1], ra)                 # and the reverse
    _, rb, _ = OracleScene(motion.deformed_description(sd, {k: (vb, nb)})).render(lp, records=True, threads=8)
    _same(g.render(lp, records=True)[1], rb)
    c2 = g.clone()                                           # a clone of an updated handle renders the updated geometry
    _same(c2.render(lp, records=True)[1], rb)
    g.update_vertices(k, va, na)
    _same(c2.render(lp, records=True)[1], rb)
    _same(g.render(lp, records=True)[1], ra)
    c2.update_vertices(k, _verts(sd, k), np.ctypeslib.as_array(sd.shapes[k].normals, shape=(sd.shapes[k].n_vertices, 3)).copy())
    _same(c2.render(lp, records=True)[1], r0)                # back to the vertices as described
    g.close()
    _same(c.render(lp, records=True)[1], ra)


def test_rolling_sequence_around_an_update(hiplib):
    pytest.importorskip("torch")
    sd, lp = _multi_mesh(False)
    k = _target(sd)
    v, n = deform(sd, k, "twist")
    g = capi.Scene(sd)
    seeds = [21, 22, 23, 24]
    seq = _Sequence(g, lp, seeds)
    seq.issue([0, 1])
    g.update_vertices(k, v, n)
    seq.issue([2, 3])
    g.flush()
    h, recs = seq.results()
    new_sd = motion.deformed_description(sd, {k: (v, n)})
    old, new = OracleScene(sd), OracleScene(new_sd)
    for i, seed in enumerate(seeds):
        li = _launch_like(lp, seed)
        ho, ro, so, add = (old if i < 2 else new).render(li, records=True, threads=8, addends=True)
        _same(recs[i], ro)
        assert_fp32_sum(h[i], add.ref, add.S, add.N, f"rolling render {i}", counts=count_channels(li, sd if i < 2 else new_sd))


def test_device_forms_and_the_bound(hiplib):
    torch = pytest.importorskip("torch")
    sd, lp = _multi_mesh(True)
    k = _target(sd)
    v, n = deform(sd, k, "twist")
    h = capi.Scene(sd)
    h.update_vertices(k, v, n)
    _, rh, _ = h.render(lp, records=True)
    g = capi.Scene(sd)
    stream = torch.cuda.Stream()
    dv, dn = torch.from_numpy(v).cuda(), torch.from_numpy(n).cuda()
    torch.cuda.synchronize()
    bound = float(np.abs(v).max())
    with torch.cuda.stream(stream):
        g.update_vertices_device(k, dv.data_ptr(), dn.data_ptr(), bound, stream=stream.cuda_stream)
    g.sync()
    hg, rg, _ = g.render(lp, records=True)
    _same(rg, rh)
    _oracle_check(motion.deformed_description(sd, {k: (v, n)}), lp, hg, rg, "device form")
    # a bound smaller than the data: counted by the kernel, which runs to completion; reported once by bf_scene_sync
    v2, n2 = deform(sd, k, "ripple")
    dv2, dn2 = torch.from_numpy(v2).cuda(), torch.from_numpy(n2).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g.update_vertices_device(k, dv2.data_ptr(), dn2.data_ptr(), 0.5 * float(np.abs(v2).max()), stream=stream.cuda_stream)
    with pytest.raises(capi.BeifongError) as e:
        g.sync()
    assert "status %d" % capi.BF_ERR_DEVICE in str(e.value) and "shape %d" % k in str(e.value)
    g.sync()                                                 # cleared once reported
    bad = v2.copy()
    bad[7, 1] = np.nan
    dbad = torch.from_numpy(bad).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        g.update_vertices_device(k, dbad.data_ptr(), dn2.data_ptr(), 2.0 * float(np.abs(v2).max()), stream=stream.cuda_stream)
    with pytest.raises(capi.BeifongError) as e:
        g.sync()
    assert "status %d" % capi.BF_ERR_DEVICE in str(e.value)
    # after a valid update the handle renders the oracle's records again
    with torch.cuda.stream(stream):
        g.update_vertices_device(k, dv2.data_ptr(), dn2.data_ptr(), float(np.abs(v2).max()), stream=stream.cuda_stream)
    g.sync()
    hg2, rg2, _ = g.render(lp, records=True)
    _oracle_check(motion.deformed_description(sd, {k: (v2, n2)}), lp, hg2, rg2, "after a refused update")


def _status(hiplib, g, shape, pos, nrm=None):
    return hiplib.bf_scene_update_vertices(g.handle, shape, pos.ctypes.data_as(C.c_void_p) if pos is not None else None,
                                           nrm.ctypes.data_as(C.c_void_p) if nrm is not None else None, None)


def test_errors_leave_the_scene_intact(hiplib):
    sd, lp = _multi_mesh(True)
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    k = _target(sd)
    plain = next(m for m in _meshes(sd) if not _has_normals(sd, m))
    rect = next(i for i, s in enumerate(sd.shapes) if s.type != capi.BF_SHAPE_MESH)
    v, n = deform(sd, k, "ripple")
    nan, inf_n = v.copy(), n.copy()
    nan[3, 2] = np.nan
    inf_n[5, 0] = np.inf
    vp = _verts(sd, plain)
    for args in [(rect, v), (len(sd.shapes), v), (k, None), (k, nan), (k, v, inf_n), (plain, vp, vp)]:
        assert _status(hiplib, g, *args) == capi.BF_ERR_INVALID, args[0]
        assert "shape %d" % args[0] in hiplib.bf_last_error().decode() or args[1] is None
    for bound in (0.0, -1.0, float("nan"), float("inf")):
        st = hiplib.bf_scene_update_vertices_device(g.handle, k, C.c_void_p(4096), None, C.c_float(bound), None)
        assert st == capi.BF_ERR_INVALID
    # batches: a shape listed twice, no renders, a multi-pixel film, a rolling launch
    k3 = np.ascontiguousarray(np.stack([v, v]))
    shapes2 = np.array([k, k], np.uint32)
    ptrs = (C.c_void_p * 2)(k3.ctypes.data, k3.ctypes.data)
    hist = np.zeros((2, g.channels(lp)), f32)

    def batch(launch, n_renders, n_deform):
        return hiplib.bf_render_deform_batch(g.handle, C.byref(launch), n_renders, None, n_deform, shapes2.ctypes.data_as(C.c_void_p), ptrs, None,
                                             0, None, hist.ctypes.data_as(C.c_void_p), None, None)
    assert batch(lp, 2, 2) == capi.BF_ERR_INVALID and "twice" in hiplib.bf_last_error().decode()
    assert batch(lp, 0, 1) == capi.BF_ERR_INVALID
    assert batch(_with_flags(lp, capi.BF_FLAG_ROLLING), 2, 1) == capi.BF_ERR_INVALID
    film = _launch_like(lp, lp.seed)
    film.spp, film.film_width, film.film_height = 1, 2, 2
    assert batch(film, 2, 1) == capi.BF_ERR_INVALID
    # the batch's own refusals: the bound of the device form, a non-mesh shape, an index out of range; render and shape named
    one = (C.c_void_p * 1)(4096)
    hdev = C.c_void_p(4096)

    def batch_dev(shape, bound, xf=None, n_renders=2):
        sh = np.array([shape], np.uint32)
        return hiplib.bf_render_deform_batch_device(g.handle, C.byref(lp), n_renders, None, 1, sh.ctypes.data_as(C.c_void_p), one, None,
                                                    C.c_float(bound), len(sd.shapes) if xf is not None else 0,
                                                    xf.ctypes.data_as(C.c_void_p) if xf is not None else None, hdev, None, None, None)
    for bound in (0.0, -2.0, float("nan"), float("inf")):
        assert batch_dev(k, bound) == capi.BF_ERR_INVALID and "bound" in hiplib.bf_last_error().decode()
    assert batch_dev(rect, 10.0) == capi.BF_ERR_INVALID and "shape %d" % rect in hiplib.bf_last_error().decode()
    assert batch_dev(len(sd.shapes), 10.0) == capi.BF_ERR_INVALID and "shape %d" % len(sd.shapes) in hiplib.bf_last_error().decode()
    xf = np.ascontiguousarray(np.tile(_identity(sd)[None], (2, 1, 1, 1)).astype(f32))
    xf[1, k, 0, 0] = 1.5                                     # render 1, shape k: not rigid
    assert batch_dev(k, 10.0, xf) == capi.BF_ERR_INVALID
    msg = hiplib.bf_last_error().decode()
    assert "render 1" in msg and "shape %d" % k in msg
    nanpos = np.ascontiguousarray(np.stack([v, nan]))
    ptr1 = (C.c_void_p * 1)(nanpos.ctypes.data)
    st = hiplib.bf_render_deform_batch(g.handle, C.byref(lp), 2, None, 1, np.array([k], np.uint32).ctypes.data_as(C.c_void_p), ptr1, None, 0, None,
                                       hist.ctypes.data_as(C.c_void_p), None, None)
    assert st == capi.BF_ERR_INVALID
    msg = hiplib.bf_last_error().decode()
    assert "render 1" in msg and "shape %d" % k in msg
    _same(g.render(lp, records=True)[1], r0)
    # a mesh that carries an emitter: unsupported, named in the message
    sd2, lp2 = _multi_mesh(False)
    m0 = _meshes(sd2)[0]
    sd2.shapes[m0].emitter = 0
    sd2.finalize()
    g2 = capi.Scene(sd2)
    _, q0, _ = g2.render(lp2, records=True)
    with pytest.raises(capi.BeifongError) as e:
        g2.update_vertices(m0, _verts(sd2, m0))
    assert "status %d" % capi.BF_ERR_UNSUPPORTED in str(e.value) and "shape %d" % m0 in str(e.value)
    p2 = np.ascontiguousarray(np.stack([_verts(sd2, m0)] * 2))
    with pytest.raises(capi.BeifongError) as e:
        g2.render_deform_batch(lp2, {m0: p2})
    assert "status %d" % capi.BF_ERR_UNSUPPORTED in str(e.value) and "shape %d" % m0 in str(e.value)
    _same(g2.render(lp2, records=True)[1], q0)


def test_next_render_reports_a_violation(hiplib):
    """a render issued right after a bad device update is the one that reports it; the one after that is clean again"""
    torch = pytest.importorskip("torch")
    sd, lp = _multi_mesh(False)
    k = _target(sd)
    v, _ = deform(sd, k, "ripple")
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    dv = torch.from_numpy(v).cuda()
    torch.cuda.synchronize()
    g.update_vertices_device(k, dv.data_ptr(), None, 0.25 * float(np.abs(v).max()))
    with pytest.raises(capi.BeifongError) as e:
        g.render(lp, records=True)
    assert "status %d" % capi.BF_ERR_DEVICE in str(e.value) and "shape %d" % k in str(e.value)
    g.render(lp)                                             # reported once
    g.update_vertices_device(k, dv.data_ptr(), None, float(np.abs(v).max()))
    hg, rg, _ = g.render(lp, records=True)
    _oracle_check(motion.deformed_description(sd, {k: v}), lp, hg, rg, "after the report")
    assert not np.array_equal(rg["L"], r0["L"])


def test_mitsuba_layer_parameters_changed(mitsuba, hiplib, tmp_path):
    """Load a scene with a PLY mesh, set_vertex_positions (+ normals) + parameters_changed, render: the film is that of a scene
    loaded from the same mesh written with the new vertices, per path too, and the cached device handle was updated, not created
    again.  Films are atomic sums: both are held to the oracle's fp32 summation bound on the second scene's description."""
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_gpu_host import RADAR_MESH_SCENE, _write_ply_be
    v, f, n = scenes.bus_mesh(20000)
    v = np.ascontiguousarray(v, f32)
    c = 0.5 * (v.min(0) + v.max(0))
    v2 = np.ascontiguousarray(((v - c) * np.array([1.0, 0.8, 1.3], f32) + c + 0.05 * np.sin(7.0 * v[:, ::-1])).astype(f32))
    n2 = np.ascontiguousarray(meshgen.vertex_normals(v2, f), f32)
    _write_ply_be(tmp_path / "a.ply", v, f, normals=n)
    _write_ply_be(tmp_path / "b.ply", v2, f, normals=n2)
    a = load_string(RADAR_MESH_SCENE % ("ply", "a.ply", ""), base_dir=str(tmp_path))
    b = load_string(RADAR_MESH_SCENE % ("ply", "b.ply", ""), base_dir=str(tmp_path))
    sa, sb = a.sensors()[0], b.sensors()[0]
    a.integrator().render(a, sa)                             # the device scene exists now
    film0 = np.array(sa.film().bitmap(raw=True)).reshape(-1).copy()
    assert a.device_creations() == 1
    mesh_a, mesh_b = a.shapes()[2], b.shapes()[2]
    assert np.array_equal(mesh_a.vertex_positions_buffer(), v.reshape(-1))
    mesh_a.set_vertex_positions(mesh_b.vertex_positions_buffer())
    mesh_a.set_vertex_normals(mesh_b.vertex_normals_buffer())         # as the loader normalised them
    mesh_a.parameters_changed()
    a.integrator().render(a, sa)
    assert a.device_creations() == 1                         # updated through bf_scene_update_vertices, not rebuilt
    film_a = np.array(sa.film().bitmap(raw=True)).reshape(-1)
    b.integrator().render(b, sb)
    film_b = np.array(sb.film().bitmap(raw=True)).reshape(-1)
    assert b.device_creations() == 1
    lp = b.integrator().launch_for(sb)
    desc_b = b.flat_desc(sb)
    ho, ro, so, add = OracleScene(desc_b).render(lp, records=True, threads=8, addends=True)
    for film, what in ((film_a, "updated scene"), (film_b, "reloaded scene")):
        assert_fp32_sum(film, add.ref, add.S, add.N, what, counts=count_channels(lp, desc_b))
    assert film_a[4] == film_b[4] == lp.n_paths and not np.array_equal(film_a, film0)
    # per path, on the handle the integrator renders with
    ga = capi.Scene.borrow(_host.lib().bfh_scene_device(a._ptr, sa._ptr), owner=a)
    _same(ga.render(lp, records=True)[1], ro)
    assert a.device_creations() == 1
    with pytest.raises(_host.HostError):
        a.shapes()[1].parameters_changed()                   # a rectangle


def test_vibrating_plate_sidebands(hiplib):
    """A plate facing the radar, every vertex displaced along the line of sight by A sin(2 pi k / 16) over 64 pulses: the phase
    of the return is modulated at 4 cycles per sweep, so the strongest lines away from zero Doppler are slow-time bins +-4.
    4 pi A / wavelength = 0.8 < 1: the first Bessel sidebands dominate the higher ones (J1 = 0.37, J2 = 0.076, J3 = 0.010)."""
    pytest.importorskip("torch")
    from beifong_amd import sweep
    lam, n_pulses = 0.1, 64
    amp = 0.8 * lam / (4.0 * np.pi)
    sd, lp = scenes.plate_doppler(wavelength_m=lam, n_paths=1 << 16, ground=False)
    k = _meshes(sd)[0]
    p = _verts(sd, k)
    axis = 0                                                 # the plate stands at x = 5 and faces the radar along x
    pos = np.tile(p[None], (n_pulses, 1, 1))
    pos[:, :, axis] = (p[None, :, axis].astype(np.float64) + amp * np.sin(2.0 * np.pi * np.arange(n_pulses) / 16.0)[:, None]).astype(f32)
    cube = sweep.render_deform_sweep(sd, lp, {k: np.ascontiguousarray(pos)}, n_streams=2)
    still = sweep.render_deform_sweep(sd, lp, {k: np.ascontiguousarray(np.tile(p[None], (n_pulses, 1, 1)))}, n_streams=2)
    assert cube.shape == (n_pulses, 1, 3) and np.all(cube[:, 0, 2] == lp.n_paths)
    rd = np.abs(sweep.range_doppler(cube, window=False)[:, 0])
    rs = np.abs(sweep.range_doppler(still, window=False)[:, 0])
    away = np.argsort(rd[1:])[::-1] + 1                      # non-zero Doppler bins, strongest first
    assert {int(away[0]), int(away[1])} == {4, n_pulses - 4}, away[:6]
    # levels against the static plate of the same test: the sidebands stand far above what it has there, and the carrier drops
    assert min(rd[4], rd[n_pulses - 4]) > 10.0 * max(rs[4], rs[n_pulses - 4], np.median(rs[1:]))
    assert rd[0] < rs[0]
    assert max(rd[8], rd[n_pulses - 8]) < min(rd[4], rd[n_pulses - 4])
