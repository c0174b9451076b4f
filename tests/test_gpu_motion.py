"""Per-mesh rigid motion (bf_scene_transform_meshes): every mesh moves by its own 3x4, the BVHs are re-fitted on the
device, and every path renders bit-identically to a scene created from the moved vertices (motion.apply_rigid) — closest hits do
not depend on the accelerator, the refitted boxes only decide which triangles are tested."""
import ctypes as C
import os

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, scenes
from beifong_amd.scenedesc import SceneDesc
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _launch_like, _same_records

pytestmark = pytest.mark.gpu
MESH = capi.BF_SHAPE_MESH


def _meshes(sd):
    return [k for k, s in enumerate(sd.shapes) if s.type == MESH]


def _centre(sd, k):
    s = sd.shapes[k]
    p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).astype(np.float64)
    return 0.5 * (p.min(0) + p.max(0))


def _identity(sd):
    return np.tile(motion.rigid(), (len(sd.shapes), 1, 1))


def _poses(sd, variant=0):
    """Every mesh its own motion about its own centre: a 90 degree turn, a 180 degree yaw, a tilted turn, each with a shift."""
    xf = _identity(sd)
    turns = [([0, 0, 1], 90.0, (0.4, -0.3, 0.0)), ([0, 0, 1], 180.0, (-0.5, 0.2, 0.0)), ([1, 0.5, 3], 30.0, (0.3, 0.6, 0.05))]
    for i, k in enumerate(_meshes(sd)):
        axis, deg, t = turns[(i + variant) % len(turns)]
        xf[k] = motion.about(motion.rotation(axis, deg + 7.0 * variant), _centre(sd, k), t)
    return xf


def _multi_mesh(normals):
    """scenes.multi_mesh_radar at 2 % size; normals=True: the car carries vertex normals"""
    if not normals:
        return scenes.multi_mesh_radar(n_paths=1 << 15, bins=1024, dr=0.03, scale=0.02)
    sd = SceneDesc()
    scenes._radar_frontend(sd)
    scenes._ground(sd)
    mat = sd.add_roughconductor(alpha=0.1, twosided=True, specular_reflectance=1.0)
    v, f = meshgen.bus(4000, seed=1)
    sd.add_mesh(meshgen.place(v, -20.0, (12.0, 3.0, 1.7)), f, mat)
    v, f, n = meshgen.car_body(20000, seed=2, with_normals=True)
    sd.add_mesh(meshgen.place(v, 15.0, (7.0, -2.5, 0.75)), f, mat, normals=meshgen.vertex_normals(meshgen.place(v, 15.0, (7.0, -2.5, 0.75)), f))
    v, f = meshgen.motorbike(6000, seed=5)
    sd.add_mesh(meshgen.place(v, 40.0, (5.0, 1.0, 0.0)), f, mat)
    sd.finalize()
    return sd, capi.make_launch(capi.BF_MODE_RANGE, 1 << 15, seed=3, bins=1024, bin_width=0.03)


def _receive_iq():
    sd, lp = scenes.bus_receive(n_tris=20000, n_paths=40000)
    lp.mode = capi.BF_MODE_RECEIVE_IQ
    return sd, lp


def _with_flags(lp, flags):
    return _launch_like(lp, lp.seed, flags=lp.flags | flags)


def _same(a, b):
    _same_records(a, b)


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("case", ["range", "range_normals", "receive_iq"])
def test_transform_equals_rebuilt_scene(hiplib, case, fast):
    sd, lp = _receive_iq() if case == "receive_iq" else _multi_mesh(case == "range_normals")
    lp = _with_flags(lp, capi.BF_FLAG_FAST if fast else 0)
    xf = _poses(sd)
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    box0 = [list(g.info().bbox_min), list(g.info().bbox_max)]
    g.transform_meshes(xf)
    hg, rg, sg = g.render(lp, records=True)
    assert [list(g.info().bbox_min), list(g.info().bbox_max)] == box0      # bf_scene_info keeps the box as created
    fresh_sd = motion.moved_description(sd, xf)
    hf, rf, sf = capi.Scene(fresh_sd).render(lp, records=True)
    _same(rg, rf)
    assert sg.n_rays_closest == sf.n_rays_closest and sg.n_rays_shadow == sf.n_rays_shadow
    assert not np.array_equal(rg["L"], r0["L"])             # the motion shows
    if not fast:
        ho, ro, so, add = OracleScene(fresh_sd).render(lp, records=True, threads=8, addends=True)
        _same(rg, ro)
        assert_fp32_sum(hg, add.ref, add.S, add.N, f"{case} moved", counts=count_channels(lp, fresh_sd))


def test_transform_is_absolute(hiplib):
    """A then B == B alone; the identity restores the records as created; translate(o) after a transform == p0 + o."""
    sd, lp = _multi_mesh(True)
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    a, b = _poses(sd, 0), _poses(sd, 1)
    g.transform_meshes(a)
    g.transform_meshes(b)
    _, rab, _ = g.render(lp, records=True)
    _, rb, _ = capi.Scene(motion.moved_description(sd, b)).render(lp, records=True)
    _same(rab, rb)
    g.transform_meshes({})                                   # every shape back to the identity
    _, ri, _ = g.render(lp, records=True)
    _same(ri, r0)
    g.transform_meshes(a)
    off = [0.3, -0.2, 0.05]
    g.translate_meshes(off)
    _, rt, _ = g.render(lp, records=True)
    ref = capi.Scene(sd)
    ref.translate_meshes(off)
    _, rr, _ = ref.render(lp, records=True)
    _same(rt, rr)
    xo = _identity(sd)
    for k in _meshes(sd):
        xo[k] = motion.rigid(t=off)
    _, rf, _ = capi.Scene(motion.moved_description(sd, xo)).render(lp, records=True)
    _same(rt, rf)


def _rays_at(sd, xf, n, seed):
    """Rays from the radar (0, 0, 0.3) and random rays through each moved mesh's box."""
    rng = np.random.default_rng(seed)
    rays = []
    for k in _meshes(sd):
        s = sd.shapes[k]
        p, _ = motion.apply_rigid(np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)), None, xf[k])
        lo, hi = p.min(0), p.max(0)
        for origin in ("radar", "random"):
            tgt = lo + rng.random((n, 3)) * (hi - lo)
            if origin == "radar":
                o = np.tile(np.array([0.0, 0.0, 0.3]), (n, 1))
            else:
                o = tgt + rng.normal(size=(n, 3)) * 5.0
            d = tgt - o
            d /= np.linalg.norm(d, axis=1, keepdims=True)
            r = np.zeros((n, 8), np.float32)
            r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 0.0, d, np.inf
            rays.append(r)
    return np.concatenate(rays)


def test_ray_queries_match_rebuilt_scene(hiplib):
    sd, _ = _multi_mesh(True)
    xf = _poses(sd)
    g = capi.Scene(sd)
    g.transform_meshes(xf)
    rays = _rays_at(sd, xf, 12000, 5)
    assert rays.shape[0] >= 64000
    a = g.ray_intersect(rays)
    b = capi.Scene(motion.moved_description(sd, xf)).ray_intersect(rays)
    assert np.array_equal(a["raw"].view(np.uint32), b["raw"].view(np.uint32))
    assert np.array_equal(a["prim"], b["prim"]) and np.array_equal(a["shape"], b["shape"])
    assert np.isfinite(a["t"]).mean() > 0.3                    # most rays do hit something


@pytest.mark.parametrize("knob", [{"BF_NO_WIDE_BVH": "1"}, {"BF_QUANT_BVH": "1"}], ids=["no_wide", "quant"])
def test_tree_variants(hiplib, monkeypatch, knob):
    """The knobs are read when a handle is created: the refit of the four-wide tree alone, and the re-quantised wf_trace nodes."""
    for k, v in knob.items():
        monkeypatch.setenv(k, v)
    for sd, lp in (_multi_mesh(True), _receive_iq()):
        xf = _poses(sd, 2)
        g = capi.Scene(sd)
        if "BF_QUANT_BVH" in knob:
            assert g.info().trace_node_bytes == 64
        g.transform_meshes(xf)
        _, rg, _ = g.render(lp, records=True)
        _, rf, _ = capi.Scene(motion.moved_description(sd, xf)).render(lp, records=True)
        _same(rg, rf)


def test_clones_copy_on_write(hiplib):
    """A transformed clone leaves its source's renders (normals included) as they were, and the other way round."""
    sd, lp = _multi_mesh(True)
    a, b = _poses(sd, 0), _poses(sd, 1)
    g = capi.Scene(sd)
    c = g.clone()
    _, r0, _ = g.render(lp, records=True)
    c.transform_meshes(a)
    _, rc, _ = c.render(lp, records=True)
    _, rg, _ = g.render(lp, records=True)
    _same(rg, r0)
    _, ra, _ = capi.Scene(motion.moved_description(sd, a)).render(lp, records=True)
    _same(rc, ra)
    g.transform_meshes(b)
    _, rc2, _ = c.render(lp, records=True)
    _same(rc2, ra)
    _, rb, _ = capi.Scene(motion.moved_description(sd, b)).render(lp, records=True)
    _, rg2, _ = g.render(lp, records=True)
    _same(rg2, rb)
    # a clone of a moved handle starts from what that handle renders now, and keeps it when the source moves on
    c2 = g.clone()
    _, rc3, _ = c2.render(lp, records=True)
    _same(rc3, rb)
    g.transform_meshes({})
    _, rc4, _ = c2.render(lp, records=True)
    _same(rc4, rb)
    _, rg3, _ = g.render(lp, records=True)
    _same(rg3, r0)
    g.close()
    _, rc5, _ = c.render(lp, records=True)
    _same(rc5, ra)


def test_rolling_sequence_around_a_transform(hiplib):
    """Rolling renders issued before a transform are renders of the old pose, those after it of the new one."""
    pytest.importorskip("torch")
    sd, lp = _multi_mesh(False)
    xf = _poses(sd)
    g = capi.Scene(sd)
    seeds = [21, 22, 23, 24]
    seq = _Sequence(g, lp, seeds)
    seq.issue([0, 1])
    g.transform_meshes(xf)
    seq.issue([2, 3])
    g.flush()
    h, recs = seq.results()
    old, new = capi.Scene(sd), capi.Scene(motion.moved_description(sd, xf))
    for k, seed in enumerate(seeds):
        ref = old if k < 2 else new
        hs, rs, ss = ref.render(_launch_like(lp, seed), records=True)
        _same(recs[k], rs)
        assert h[k][4] == hs[4] == lp.n_paths - ss.n_invalid


def test_batch_offsets_on_top_of_a_transform(hiplib):
    sd, lp = _receive_iq()
    xf = _poses(sd)
    g = capi.Scene(sd)
    g.transform_meshes(xf)
    offs = np.array([[0.0, 0.0, 0.0], [0.25, -0.1, 0.0], [-0.5, 0.3, 0.02]], np.float32)
    _, rb, _ = g.render_batch(lp, len(offs), offsets=offs, records=True)
    moved = motion.moved_description(sd, xf)
    k_mesh = _meshes(sd)[0]
    for i, off in enumerate(offs):
        xo = _identity(sd)
        xo[k_mesh] = motion.rigid(t=off)
        s = moved.shapes[k_mesh]
        p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3))
        p2 = (p + off[None, :]).astype(np.float32)          # fl(p' + off)
        fresh = motion.moved_description(moved, xo)
        q = np.ctypeslib.as_array(fresh.shapes[k_mesh].positions, shape=(s.n_vertices, 3))
        if not np.any(off):
            q = p
        assert np.array_equal(q, p2)
        _, rf, _ = capi.Scene(fresh).render(lp, records=True)
        _same(rb[i], rf)


def test_errors_leave_the_scene_intact(hiplib):
    sd, lp = _multi_mesh(True)
    g = capi.Scene(sd)
    good = _poses(sd)
    g.transform_meshes(good)
    _, r0, _ = g.render(lp, records=True)
    k = _meshes(sd)[1]
    rect = next(i for i, s in enumerate(sd.shapes) if s.type != MESH and s.emitter < 0)
    scale = good.copy()
    scale[k, :, :3] *= np.float32(1.01)
    shear = good.copy()
    shear[k, 0, 1] += np.float32(0.05)
    mirror = good.copy()
    mirror[k, :, 0] *= -1
    nan = good.copy()
    nan[k, 1, 3] = np.nan
    on_rect = good.copy()
    on_rect[rect] = motion.rigid(t=(0.0, 0.0, 0.1))
    cases = [(scale, capi.BF_ERR_INVALID), (shear, capi.BF_ERR_INVALID), (mirror, capi.BF_ERR_INVALID), (nan, capi.BF_ERR_INVALID),
             (on_rect, capi.BF_ERR_INVALID)]
    for xf, want in cases:
        st = hiplib.bf_scene_transform_meshes(g.handle, xf.shape[0], np.ascontiguousarray(xf).ctypes.data_as(C.c_void_p), None)
        assert st == want
    st = hiplib.bf_scene_transform_meshes(g.handle, len(sd.shapes) - 1, np.ascontiguousarray(good).ctypes.data_as(C.c_void_p), None)
    assert st == capi.BF_ERR_INVALID
    _, r1, _ = g.render(lp, records=True)
    _same(r1, r0)
    # a moved mesh that carries an emitter (its triangles evaluate the radar's emitter): unsupported, named in the message
    sd2, lp2 = _multi_mesh(False)
    sd2.shapes[_meshes(sd2)[0]].emitter = 0
    sd2.finalize()
    g2 = capi.Scene(sd2)
    _, q0, _ = g2.render(lp2, records=True)
    xf2 = _poses(sd2)
    with pytest.raises(capi.BeifongError) as e:
        g2.transform_meshes(xf2)
    assert "status %d" % capi.BF_ERR_UNSUPPORTED in str(e.value) and "shape %d" % _meshes(sd2)[0] in str(e.value)
    _, q1, _ = g2.render(lp2, records=True)
    _same(q1, q0)


def _two_plates(v_a, v_b):
    """plate_doppler with a second, smaller plate beside the first; returns (sd, lp, [plate meshes])"""
    sd, lp = scenes.plate_doppler(wavelength_m=0.1, n_paths=1 << 16, ground=True)
    k0 = _meshes(sd)[0]
    s = sd.shapes[k0]
    p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()
    f = np.ctypeslib.as_array(s.indices, shape=(s.n_faces, 3)).copy()
    p2 = p.copy()
    p2[:, 1] += 1.0          # beside the first plate, same range: returns of comparable strength
    sd.add_mesh(p2, f, sd.add_diffuse(0.8, twosided=True))
    sd.finalize()
    return sd, lp, [k0, len(sd.shapes) - 1]


def test_two_targets_range_doppler(hiplib):
    """Two plates approaching at different speeds, one motion sweep: two Doppler lines where the speeds put them."""
    pytest.importorskip("torch")
    from beifong_amd import sweep
    lam, n_pulses = 0.1, 64
    dx = {0: -0.004, 1: -0.0125}
    sd, lp, plates = _two_plates(*dx.values())
    xf = np.tile(_identity(sd)[None], (n_pulses, 1, 1, 1))
    for i, k in enumerate(plates):
        xf[:, k, 0, 3] = dx[i] * np.arange(n_pulses)
    cube = sweep.render_motion_sweep(sd, lp, xf, n_streams=2)
    assert cube.shape == (n_pulses, 1, 3) and np.all(cube[:, 0, 2] == lp.n_paths)
    rd = np.abs(sweep.range_doppler(cube)[:, 0])
    order = np.argsort(rd)[::-1]
    top = {int(x) for x in order[:8]}             # four per line, as test_pulse_sweep_range_doppler_peak allows one
    floor = np.median(rd)
    for i in range(2):
        expect = int(round(2 * abs(dx[i]) / lam * n_pulses)) % n_pulses
        assert expect in top or (expect + 1) % n_pulses in top, (i, expect, sorted(top))
        assert max(rd[expect], rd[(expect + 1) % n_pulses]) > 10 * floor
    # one pulse against a stand-alone transformed render
    k = 17
    g = capi.Scene(sd)
    g.transform_meshes(xf[k])
    h_k, _, _ = g.render(lp)
    assert np.allclose(h_k.reshape(1, 3), cube[k], rtol=1e-4, atol=1e-6 * np.abs(cube[k]).max())
