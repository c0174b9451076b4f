"""Device-side BSDF, emitter, sensor and ray queries (include/beifong_hip.h: "plugin-level queries on the device") held to the
oracle path by path: the same functions the render kernels call, bit for bit against the oracle's bfo_* entries, plus the
reference's own per-plugin known answers (tests/test_oracle_known_answers.py, tests/test_oracle_chi2.py) rerun on the device."""
import ctypes as C
import math

import numpy as np
import pytest

from beifong_amd import capi, motion, scenes
from beifong_amd.scenedesc import SceneDesc, Transform4f
from tests.oracle_lib import OracleScene
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.rolling_helpers import _Sequence, _launch_like, _same_records
from tests.scene_builders import _fuzz_scene

pytestmark = pytest.mark.gpu

f32 = np.float32
T = Transform4f


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def olib():
    from tests import oracle_lib
    lib = oracle_lib.load()
    lib.bfo_material_for_side.argtypes = [C.c_void_p, C.c_uint32, C.c_float]
    lib.bfo_material_for_side.restype = C.c_uint32
    lib.bfo_microfacet.argtypes = [C.c_int, C.c_uint32, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float,
                                   C.c_void_p]
    lib.bfo_microfacet.restype = None
    return lib


def _material_scene(materials):
    """A scene whose material table is exactly `materials` (one rectangle per entry), a point light and a camera."""
    sd = SceneDesc()
    for k, m in enumerate(materials):
        sd.materials.append(m)
        sd.add_rectangle(T.translate([3.0 * k, 0, 0]), k)
    sd.add_point([0, 0, 5], intensity=1.0)
    sd.set_perspective(T.translate([0, 0, 5]), fov=45.0)
    sd.finalize()
    return sd


def _directions(n, rng):
    """Unit vectors over the whole sphere, a share of them grazing (|z| < 1e-3, z = 0 and z = +-1e-7 included)."""
    v = rng.normal(size=(n, 3))
    g = n // 8
    v[:g, 2] = rng.uniform(-1e-3, 1e-3, g) * np.linalg.norm(v[:g, :2], axis=1)
    v[g:g + 4, 2] = [0.0, 1e-7, -1e-7, 0.0]
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v.astype(f32)


def _oracle_eval_pdf(olib, table, k, wi, wo):
    j = olib.bfo_material_for_side(table, k, float(wi[2]))
    m = C.byref(table[j])
    return olib.bfo_bsdf_eval(m, _p(wi), _p(wo)), olib.bfo_bsdf_pdf(m, _p(wi), _p(wo))


def _table_cases():
    cases = []
    for seed in range(8):
        sd, _ = _fuzz_scene(seed)
        cases.append((f"fuzz{seed}", sd))
    sd = SceneDesc()
    front = sd.add_diffuse(0.1)
    back = sd.add_roughconductor(alpha=0.2, distribution="ggx")
    sd.set_back_material(front, back)
    for k in range(2):
        sd.add_rectangle(T.translate([3.0 * k, 0, 0]), k)
    sd.add_point([0, 0, 5])
    sd.set_perspective(T.translate([0, 0, 5]))
    sd.finalize()
    cases.append(("back_material", sd))
    return cases


TABLES = _table_cases()


@pytest.mark.parametrize("name,sd", TABLES, ids=[c[0] for c in TABLES])
def test_bsdf_eval_pdf_bit_equal_to_oracle(hiplib, olib, name, sd):
    g = capi.Scene(sd)
    table = (capi.bf_material * len(sd.materials))(*sd.materials)
    rng = np.random.default_rng(sum(map(ord, name)))
    n = 4096
    for k in range(len(sd.materials)):
        wi, wo = _directions(n, rng), _directions(n, rng)
        rows = np.concatenate([wi, wo], 1)
        got = g.bsdf_eval_pdf(np.full(n, k, np.uint32), rows)
        ref = np.array([_oracle_eval_pdf(olib, table, k, wi[i], wo[i]) for i in range(n)], f32)
        assert np.array_equal(_bits(got), _bits(ref)), (name, k, np.flatnonzero((_bits(got) != _bits(ref)).any(1))[:5])


@pytest.mark.parametrize("name,sd", TABLES, ids=[c[0] for c in TABLES])
def test_bsdf_sample_bit_equal_to_oracle(hiplib, olib, name, sd):
    g = capi.Scene(sd)
    table = (capi.bf_material * len(sd.materials))(*sd.materials)
    rng = np.random.default_rng(7 + sum(map(ord, name)))
    n = 4096
    for k in range(len(sd.materials)):
        wi = _directions(n, rng)
        u = rng.random((n, 3), dtype=f32)
        got = g.bsdf_sample(np.full(n, k, np.uint32), np.concatenate([wi, u], 1))
        ref = np.zeros((n, 5), f32)
        for i in range(n):
            j = olib.bfo_material_for_side(table, k, float(wi[i, 2]))
            wo, pdf = np.zeros(3, f32), C.c_float()
            w = olib.bfo_bsdf_sample(C.byref(table[j]), _p(wi[i]), float(u[i, 0]), float(u[i, 1]), float(u[i, 2]), _p(wo), C.byref(pdf))
            ref[i] = [wo[0], wo[1], wo[2], pdf.value, w]
        assert np.array_equal(_bits(got), _bits(ref)), (name, k, np.flatnonzero((_bits(got) != _bits(ref)).any(1))[:5])


# ---- the reference's known answers, on the device -------------------------------------------------------------------
def _one(m):
    return capi.Scene(_material_scene([m]))


def test_diffuse_eval_pdf_on_device(hiplib):
    # src/bsdfs/tests/test_diffuse.py:16-39 (test_oracle_known_answers.test_diffuse_eval_pdf)
    sd = SceneDesc()
    g = _one(sd.materials[sd.add_diffuse(0.5)])
    th = np.arange(20) / 19.0 * (math.pi / 2)
    wo = np.stack([np.sin(th), np.zeros(20), np.cos(th)], 1).astype(f32)
    out = g.bsdf_eval_pdf(np.zeros(20, np.uint32), np.concatenate([np.tile(f32([0, 0, 1]), (20, 1)), wo], 1))
    for i in range(20):
        if wo[i, 2] > 0:
            assert np.isclose(out[i, 1], wo[i, 2] / math.pi, atol=1e-7) and np.isclose(out[i, 0], 0.5 * wo[i, 2] / math.pi, atol=1e-7)
        else:
            assert out[i, 0] == 0 and out[i, 1] == 0


def test_twosided_pdf_on_device(hiplib):
    # src/bsdfs/tests/test_twosided.py:43-60
    sd = SceneDesc()
    g = _one(sd.materials[sd.add_diffuse(0.5, twosided=True)])
    rows = f32([[0, 0, 1, 0, 0, 1], [0, 0, 1, 0, 0, -1], [0, 0, -1, 0, 0, -1], [0, 0, -1, 0, 0, 1]])
    pdf = g.bsdf_eval_pdf(np.zeros(4, np.uint32), rows)[:, 1]
    assert np.isclose(pdf[0], 1 / math.pi) and pdf[1] == 0 and np.isclose(pdf[2], 1 / math.pi) and pdf[3] == 0


def test_twosided_sample_eval_pdf_over_the_sphere_on_device(hiplib):
    # src/bsdfs/tests/test_twosided.py:62-100 (test_oracle_known_answers.test_twosided_sample_eval_pdf_over_the_sphere)
    sd = SceneDesc()
    front, back = sd.add_diffuse(0.1, twosided=True), sd.add_diffuse(0.9, twosided=True)
    sd.set_back_material(front, back)
    g = capi.Scene(_material_scene(sd.materials))
    n = 5
    wis, us = [], []
    for u in range(n):
        for v in range(n):
            s0, s1 = u / (n - 1.0), v / (n - 1.0)
            z = 1.0 - 2.0 * s1
            r = math.sqrt(max(0.0, 1.0 - z * z))
            wi = [r * math.cos(2 * math.pi * s0), r * math.sin(2 * math.pi * s0), z]
            for x in range(n):
                for y in range(n):
                    wis.append(wi)
                    us.append([0.5, x / (n - 1.0), y / (n - 1.0)])
    wi, u = np.array(wis, f32), np.array(us, f32)
    mats = np.zeros(len(wi), np.uint32)
    s = g.bsdf_sample(mats, np.concatenate([wi, u], 1))
    ep = g.bsdf_eval_pdf(mats, np.concatenate([wi, s[:, 0:3]], 1))
    ok = s[:, 4] > 0
    up = wi[:, 2] > 0
    assert np.allclose(s[ok, 4], np.where(up[ok], 0.1, 0.9), rtol=1e-6)
    s_value = s[:, 4] * s[:, 2] / math.pi * np.where(up, 1, -1)
    assert np.all(np.abs(s_value[ok] - ep[ok, 0]) < 1e-2) and not np.isnan(ep[ok, 0]).any()
    assert np.allclose(s[ok, 3], ep[ok, 1], rtol=1e-6)
    assert ok.sum() >= 200 and set(up[ok]) == {True, False}


def _device_microfacet(op, typ, au, av, visible, wi, m, s=(0.0, 0.0)):
    row = np.concatenate([np.asarray(wi, f32), np.asarray(m, f32), np.asarray(s, f32)]).reshape(1, 8)
    return capi.eval_microfacet(op, typ, au, av, visible, row)[0]


def test_microfacet_golden_vectors_on_device(hiplib, monkeypatch):
    """test_microfacet_distribution_golden_vectors with every MicrofacetDistribution call made by bf_eval_microfacet."""
    from tests import test_oracle_known_answers as tk
    monkeypatch.setattr(tk, "_microfacet", _device_microfacet)
    tk.test_microfacet_distribution_golden_vectors()


@pytest.mark.parametrize("typ", [capi.BF_MF_BECKMANN, capi.BF_MF_GGX])
@pytest.mark.parametrize("au,av,visible", [(0.1, 0.3, False), (0.2, 0.2, True), (0.05, 0.4, True), (0.3, 0.1, False)])
def test_microfacet_bit_equal_to_oracle(hiplib, olib, typ, au, av, visible):
    rng = np.random.default_rng(11)
    n = 2048
    wi, m = _directions(n, rng), _directions(n, rng)
    wi[:, 2] = np.abs(wi[:, 2])
    s = rng.random((n, 2), dtype=f32)
    rows = np.ascontiguousarray(np.concatenate([wi, m, s], 1))
    for op in range(4):
        got = capi.eval_microfacet(op, typ, au, av, visible, rows)
        ref = np.zeros((n, 4), f32)
        for i in range(n):
            olib.bfo_microfacet(op, typ, au, av, int(visible), _p(wi[i]), _p(m[i]), float(s[i, 0]), float(s[i, 1]), _p(ref[i]))
        cols = 4 if op == 3 else 1
        assert np.array_equal(_bits(got[:, :cols]), _bits(ref[:, :cols])), (op, np.flatnonzero((_bits(got[:, :cols]) != _bits(ref[:, :cols])).any(1))[:5])


def test_chi2_bsdf_sampling_on_device(hiplib):
    """The chi^2 fits of test_oracle_chi2.py with 10^6 device samples against device pdfs."""
    from tests.test_oracle_chi2 import CASES, _conductor, chi_square_test
    cases = [(name, _conductor(**kw), [1.0, 1.0, 1.0], tkw) for name, kw, tkw in CASES]
    sd = SceneDesc()
    sd.add_diffuse()
    cases.append(("diffuse", sd.materials[0], [0.0, 0.0, 1.0], {}))
    for name, mat, wi, tkw in cases:
        g = _one(mat)
        wi = (np.asarray(wi, np.float64) / np.linalg.norm(wi)).astype(f32)

        def sample(u):
            u = np.ascontiguousarray(u, f32)
            out = g.bsdf_sample(np.zeros(u.shape[0], np.uint32), np.concatenate([np.tile(wi, (u.shape[0], 1)), u], 1))
            return out[:, 0:3], (out[:, 4] != 0).astype(f32)

        def pdf(wo):
            wo = np.ascontiguousarray(wo, f32)
            return g.bsdf_eval_pdf(np.zeros(wo.shape[0], np.uint32), np.concatenate([np.tile(wi, (wo.shape[0], 1)), wo], 1))[:, 1]

        ok, p, msg = chi_square_test(sample, pdf, sample_dim=3, sample_count=1_000_000, **tkw)
        assert ok, (name, msg)


# ---- emitters ------------------------------------------------------------------------------------------------------
def _emitter_scene():
    sd = SceneDesc()
    floor = sd.add_rectangle(T.scale([4, 4, 1]), sd.add_diffuse(0.5))
    light = sd.add_rectangle(T.translate([0.3, -0.2, 2.0]) * T.rotate([1, 0, 0], 180) * T.scale([0.5, 0.25, 1]), sd.add_diffuse(0.0))
    sd.add_spot(T.look_at([0, 1, 3], [0, 0, 0], [1, 0, 0]), intensity=2.5, cutoff_angle=40.0)
    sd.add_point([1, -1, 2], intensity=3.0)
    sd.add_area_emitter(light, 7.0)
    sd.set_perspective(T.translate([0, 0, 5]), fov=45.0)
    sd.finalize()
    assert floor == 0
    return sd


def test_emitter_sample_direction_bit_equal_to_oracle(hiplib):
    sd = _emitter_scene()
    g, o = capi.Scene(sd), OracleScene(sd)
    rng = np.random.default_rng(3)
    n = 4096
    for k in range(len(sd.emitters)):
        rows = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.random((n, 2))], 1).astype(f32)
        got = g.emitter_sample_direction(k, rows)
        ref = np.zeros((n, 8), f32)
        for i in range(n):
            r = o.emitter_sample_direction(k, rows[i, :3], (float(rows[i, 3]), float(rows[i, 4])))
            ref[i] = [*r["d"], r["dist"], r["pdf"], float(r["delta"]), r["spec"], r["pdf_direction"]]
        assert np.array_equal(_bits(got[:, :7]), _bits(ref[:, :7])), (k, np.flatnonzero((_bits(got[:, :7]) != _bits(ref[:, :7])).any(1))[:5])
        assert np.allclose(got[:, 7], ref[:, 7], rtol=2e-6, atol=0)
        assert (got[:, 6] > 0).any()


class _DeviceEmitters:
    """Stands in for OracleScene in the emitter known-answer tests: emitter_sample_direction on the device."""

    def __init__(self, sd):
        self.g = capi.Scene(sd)

    def emitter_sample_direction(self, index, ref_p, sample=(0.0, 0.0)):
        row = np.array([[*np.asarray(ref_p, f32), sample[0], sample[1]]], f32)
        out = self.g.emitter_sample_direction(index, row)[0]
        return dict(d=out[0:3], dist=out[3], pdf=out[4], delta=bool(out[5]), spec=out[6], pdf_direction=out[7])


def test_emitter_known_answers_on_device(hiplib, monkeypatch):
    """test_oracle_known_answers.py's spot, area and point light known answers with the device doing the sampling."""
    from tests import test_oracle_known_answers as tk
    monkeypatch.setattr(tk, "OracleScene", _DeviceEmitters)
    for it_pos in ([2.0, 0.5, 0.0], [1.0, 0.5, -5.0]):
        for cutoff in (20, 80):
            for lookat in (([0, 1, 0], [0, 0, 0], [1, 0, 0]), ([0, 0, 1], [0, 0, 0], [0, -1, 0])):
                tk.test_spot_sample_direction_known_answers(it_pos, cutoff, lookat)
    tk.test_area_light_sample_direction_known_answers()
    tk.test_point_light_sample_direction_known_answers()


# ---- sensors ------------------------------------------------------------------------------------------------------
def _sensor_scene(kind):
    sd = SceneDesc()
    mat = sd.add_diffuse(0.5)
    sd.add_rectangle(T.scale([4, 4, 1]), mat)
    meter = sd.add_rectangle(T.translate([0.2, -0.1, 1.5]) * T.rotate([1, 0, 0], 160) * T.scale([0.3, 0.2, 1]), mat)
    sd.add_point([0, 0, 3])
    if kind == "perspective":
        sd.set_perspective(T.look_at([0.5, -3, 2], [0, 0, 0], [0, 0, 1]), fov=50.0, film=(64, 48), crop=(8, 4, 32, 24))
    elif kind == "fluxmeter":
        sd.set_fluxmeter(meter)
    elif kind == "irradiancemeter":
        sd.set_irradiancemeter(meter)
    else:
        sd.set_radiancemeter(T.look_at([0.5, -3, 2], [0, 0, 0], [0, 0, 1]))
    sd.finalize()
    return sd


@pytest.mark.parametrize("kind", ["perspective", "fluxmeter", "irradiancemeter", "radiancemeter"])
def test_sensor_sample_ray_bit_equal_to_oracle(hiplib, kind):
    sd = _sensor_scene(kind)
    g, o = capi.Scene(sd), OracleScene(sd)
    grid = np.linspace(0.0, 1.0, 17, dtype=f32)
    ap = np.linspace(0.05, 0.95, 4, dtype=f32)
    F = np.stack(np.meshgrid(grid, grid, ap, ap, indexing="ij"), -1).reshape(-1, 4).astype(f32)
    got = g.sensor_sample_ray(F)
    ref = np.array([[*r["o"], r["mint"], *r["d"], r["weight"]] for r in (o.sensor_sample_ray(*map(float, q)) for q in F)], f32)
    assert np.array_equal(_bits(got[:, :8]), _bits(ref)), np.flatnonzero((_bits(got[:, :8]) != _bits(ref)).any(1))[:5]
    if kind == "perspective":
        assert np.all(np.isfinite(got[:, 8]) & (got[:, 8] > got[:, 3]))
    else:
        assert np.all(np.isinf(got[:, 8]))


# ---- device forms --------------------------------------------------------------------------------------------------
def _rays(n, rng, lo=(-3, -3, 0.1), hi=(3, 3, 3)):
    o = rng.uniform(lo, hi, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.zeros((n, 8), f32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, 1e-4, d, np.inf
    return r


def _device_queries(torch, g, rays, mats, bsdf_rows, em_rows, sensor_rows, stream=0):
    """Every _device form once on `stream`; returns host copies of their outputs."""
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    n = rays.shape[0]
    t_rays, t_mats, t_b, t_e, t_s = dev(rays), dev(mats.view(np.int32)), dev(bsdf_rows), dev(em_rows), dev(sensor_rows)
    si = torch.zeros((n, capi.BF_SI_FLOATS), dtype=torch.float32, device="cuda")
    prim = torch.zeros(n, dtype=torch.int32, device="cuda")
    shape = torch.zeros(n, dtype=torch.int32, device="cuda")
    hit = torch.zeros(n, dtype=torch.uint8, device="cuda")
    ev = torch.zeros((len(mats), 2), dtype=torch.float32, device="cuda")
    sm = torch.zeros((len(mats), 5), dtype=torch.float32, device="cuda")
    em = torch.zeros((em_rows.shape[0], 8), dtype=torch.float32, device="cuda")
    sr = torch.zeros((sensor_rows.shape[0], 9), dtype=torch.float32, device="cuda")
    g.ray_intersect_device(n, t_rays.data_ptr(), si.data_ptr(), prim.data_ptr(), shape.data_ptr(), stream=stream)
    g.trace_any_device(n, t_rays.data_ptr(), hit.data_ptr(), stream=stream)
    g.bsdf_eval_pdf_device(len(mats), t_mats.data_ptr(), t_b.data_ptr(), ev.data_ptr(), stream=stream)
    g.bsdf_sample_device(len(mats), t_mats.data_ptr(), t_b.data_ptr(), sm.data_ptr(), stream=stream)
    g.emitter_sample_direction_device(0, em_rows.shape[0], t_e.data_ptr(), em.data_ptr(), stream=stream)
    g.sensor_sample_ray_device(sensor_rows.shape[0], t_s.data_ptr(), sr.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    return dict(si=si.cpu().numpy(), prim=prim.cpu().numpy().view(np.uint32), shape=shape.cpu().numpy().view(np.uint32),
                hit=hit.cpu().numpy(), ev=ev.cpu().numpy(), sm=sm.cpu().numpy(), em=em.cpu().numpy(), sr=sr.cpu().numpy())


def _host_queries(g, rays, mats, bsdf_rows, em_rows, sensor_rows):
    r = g.ray_intersect(rays)
    return dict(si=r["raw"], prim=r["prim"], shape=r["shape"], hit=g.trace_any(rays), ev=g.bsdf_eval_pdf(mats, bsdf_rows),
                sm=g.bsdf_sample(mats, bsdf_rows), em=g.emitter_sample_direction(0, em_rows), sr=g.sensor_sample_ray(sensor_rows))


def _same_outputs(a, b):
    for k in a:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k


def _query_inputs(sd, n, seed):
    rng = np.random.default_rng(seed)
    mats = rng.integers(0, len(sd.materials), n).astype(np.uint32)
    bsdf_rows = np.concatenate([_directions(n, rng), rng.random((n, 3), dtype=f32)], 1).astype(f32)
    em_rows = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.random((n, 2))], 1).astype(f32)
    sensor_rows = rng.random((n, 4), dtype=f32)
    return mats, bsdf_rows, em_rows, sensor_rows


def test_device_forms_equal_host_forms(hiplib):
    torch = pytest.importorskip("torch")
    sd, _ = scenes.trans_rad(spp=16)
    g = capi.Scene(sd)
    rays = _rays(8192, np.random.default_rng(1))
    inputs = _query_inputs(sd, 4096, 2)
    a = _host_queries(g, rays, *inputs)
    s = torch.cuda.Stream()
    b = _device_queries(torch, g, rays, *inputs, stream=s.cuda_stream)
    _same_outputs(a, b)
    assert np.isfinite(a["si"][:, 0]).any() and a["hit"].any()


def test_query_after_transform_meshes_sees_the_moved_scene(hiplib):
    torch = pytest.importorskip("torch")
    from tests.test_gpu_motion import _multi_mesh, _poses, _rays_at
    sd, _ = _multi_mesh(True)
    xf = _poses(sd)
    g = capi.Scene(sd)
    s = torch.cuda.Stream()
    g.transform_meshes(xf, stream=s.cuda_stream)
    rays = _rays_at(sd, xf, 4000, 5)
    inputs = _query_inputs(sd, 1024, 3)
    a = _device_queries(torch, g, rays, *inputs, stream=s.cuda_stream)
    b = _host_queries(capi.Scene(motion.moved_description(sd, xf)), rays, *inputs)
    _same_outputs(a, b)
    assert np.isfinite(a["si"][:, 0]).mean() > 0.3


def _endpoint_pair():
    """Two descriptions of one layout: different emitter pose and radiance, materials and camera."""
    out = []
    for v in range(2):
        sd = SceneDesc()
        sd.add_rectangle(T.scale([4, 4, 1]), sd.add_diffuse(0.5 + 0.2 * v))
        light = sd.add_rectangle(T.translate([0.3 * v, -0.2, 2.0 + v]) * T.rotate([1, 0, 0], 180) * T.scale([0.5, 0.25, 1]),
                                 sd.add_roughconductor(alpha=0.1 + 0.2 * v, distribution="ggx" if v else "beckmann"))
        sd.add_area_emitter(light, 7.0 + v)
        sd.set_perspective(T.look_at([0.5 * v, -3, 2], [0, 0, 0], [0, 0, 1]), fov=45.0 + 5 * v)
        sd.finalize()
        out.append(sd)
    return out


def test_query_after_update_endpoints_sees_the_new_endpoints(hiplib):
    torch = pytest.importorskip("torch")
    sd_a, sd_b = _endpoint_pair()
    g = capi.Scene(sd_a)
    s = torch.cuda.Stream()
    g.update_endpoints(sd_b, stream=s.cuda_stream)
    rays = _rays(4096, np.random.default_rng(4))
    inputs = _query_inputs(sd_b, 2048, 5)
    a = _device_queries(torch, g, rays, *inputs, stream=s.cuda_stream)
    b = _host_queries(capi.Scene(sd_b), rays, *inputs)
    _same_outputs(a, b)
    c = _host_queries(capi.Scene(sd_a), rays, *inputs)
    assert not np.array_equal(a["em"], c["em"]) and not np.array_equal(a["sr"], c["sr"])


def test_queries_inside_a_rolling_sequence_leave_it_unchanged(hiplib):
    """8 rolling renders with ray and BSDF queries between them (half of them after a joined endpoint update) flush to the
    same per-path records as the sequence without them — and as the oracle's stand-alone renders — and to histograms that are
    fp32 sums of those paths; the queries after the update see the new endpoints."""
    torch = pytest.importorskip("torch")
    sd_a, sd_b = _endpoint_pair()
    lp = capi.make_launch(capi.BF_MODE_RANGE, 1 << 14, seed=1, bins=256, bin_width=0.05)
    seeds = list(range(11, 19))
    rays = _rays(2048, np.random.default_rng(6))
    inputs = _query_inputs(sd_b, 1024, 7)

    def run(with_queries):
        g = capi.Scene(sd_a)
        seq = _Sequence(g, lp, seeds)
        seen = []
        for k in range(8):
            if k == 4:
                g.update_endpoints(sd_b)
            seq.issue([k])
            if with_queries:
                seen.append(_device_queries(torch, g, rays, *inputs))
        g.flush()
        h, rec = seq.results()
        return h, rec, seen

    h0, r0, _ = run(False)
    h1, r1, seen = run(True)
    # every path of every render is the same, bit for bit; the histograms are fp32 sums of those paths in the order the
    # device's atomics take them (the order differs between two runs of the same sequence, with or without queries), so each
    # is held to the oracle's exact sum within the fp32 summation bound, count channels exact
    for k in range(8):
        _same_records(r0[k], r1[k])
        l1 = _launch_like(lp, seeds[k])
        _, ro, _, add = OracleScene(sd_a if k < 4 else sd_b).render(l1, records=True, threads=8, addends=True)
        _same_records(r1[k], ro)
        counts = count_channels(l1, sd_a)
        assert_fp32_sum(h0[k], add.ref, add.S, add.N, f"sequence without queries, render {k}", counts=counts)
        assert_fp32_sum(h1[k], add.ref, add.S, add.N, f"sequence with queries, render {k}", counts=counts)
    ref_a = _host_queries(capi.Scene(sd_a), rays, *inputs)
    ref_b = _host_queries(capi.Scene(sd_b), rays, *inputs)
    for k, q in enumerate(seen):
        _same_outputs(q, ref_a if k < 4 else ref_b)


# ---- refusals ------------------------------------------------------------------------------------------------------
def test_refusals_return_their_status_and_change_nothing(hiplib):
    lib = capi.load_library()
    sd, lp = scenes.trans_rad(spp=64)
    g = capi.Scene(sd)
    before = g.render(lp, records=True)
    h = g.handle
    nm, ne = len(sd.materials), len(sd.emitters)
    row6, row5, row4, out = np.zeros((1, 6), f32), np.zeros((1, 5), f32), np.zeros((1, 4), f32), np.zeros((1, 9), f32)
    bad_mat = np.array([nm], np.uint32)
    assert lib.bf_bsdf_eval_pdf(h, 1, _p(bad_mat), _p(row6), _p(out)) == capi.BF_ERR_INVALID
    assert lib.bf_bsdf_sample(h, 1, _p(bad_mat), _p(row6), _p(out)) == capi.BF_ERR_INVALID
    assert lib.bf_emitter_sample_direction(h, ne, 1, _p(row5), _p(out)) == capi.BF_ERR_INVALID
    assert lib.bf_emitter_sample_direction_device(h, ne, 0, None, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_bsdf_eval_pdf(h, 1, None, _p(row6), _p(out)) == capi.BF_ERR_INVALID
    assert lib.bf_bsdf_sample_device(h, 1, None, None, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_sensor_sample_ray(h, 1, _p(row4), None) == capi.BF_ERR_INVALID
    assert lib.bf_ray_intersect_device(h, 1, None, None, None, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_trace_any_device(h, 1, None, None, None) == capi.BF_ERR_INVALID
    assert lib.bf_eval_microfacet(4, 0, .1, .1, 1, 1, _p(np.zeros(8, f32)), _p(out)) == capi.BF_ERR_INVALID
    assert lib.bf_eval_microfacet(0, 2, .1, .1, 1, 1, _p(np.zeros(8, f32)), _p(out)) == capi.BF_ERR_INVALID
    assert lib.bf_eval_microfacet(0, 0, .1, .1, 1, 0, None, None) == capi.BF_OK
    # n == 0: BF_OK, nothing launched, null pointers allowed
    assert lib.bf_bsdf_eval_pdf(h, 0, None, None, None) == capi.BF_OK
    assert lib.bf_sensor_sample_ray_device(h, 0, None, None, None) == capi.BF_OK
    assert lib.bf_trace_any_device(h, 0, None, None, None) == capi.BF_OK
    with pytest.raises(capi.BeifongError, match="status 1"):
        g.bsdf_eval_pdf(bad_mat, row6)
    # transmitter-type emitters and receiver-type sensors: BF_ERR_UNSUPPORTED
    sdr, _ = scenes.bus_receive(n_tris=2000, n_paths=64, t_bins=64)
    gr = capi.Scene(sdr)
    kinds = [e.type for e in sdr.emitters]
    k_tx = next(i for i, t in enumerate(kinds) if t in (capi.BF_TRANSMITTER_AREA, capi.BF_TRANSMITTER_WIGNER, capi.BF_TRANSMITTER_PHASED))
    assert lib.bf_emitter_sample_direction(gr.handle, k_tx, 1, _p(row5), _p(out)) == capi.BF_ERR_UNSUPPORTED
    assert lib.bf_emitter_sample_direction_device(gr.handle, k_tx, 1, _p(row5), _p(out), None) == capi.BF_ERR_UNSUPPORTED
    assert lib.bf_sensor_sample_ray(gr.handle, 1, _p(row4), _p(out)) == capi.BF_ERR_UNSUPPORTED
    assert lib.bf_sensor_sample_ray_device(gr.handle, 1, _p(row4), _p(out), None) == capi.BF_ERR_UNSUPPORTED
    after = g.render(lp, records=True)
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32))
    _same_records(before[1], after[1])
