"""The mitsuba-shaped layer's device queries (Scene.ray_intersect / ray_test, Shape.bsdf(), Scene.emitters()[i].sample_direction,
Sensor.sample_ray) on tests/golden/trans_rad.xml (a spot light, a fluxmeter, a twosided diffuse material) and a small scene with point and area lights: they run
on the bf_scene the integrator renders with and equal both the capi results and the oracle on the same flat description."""
import ctypes as C
import os

import numpy as np
import pytest

from beifong_amd import capi
from tests.oracle_lib import OracleScene

pytestmark = pytest.mark.gpu

f32 = np.float32
XML = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "trans_rad.xml")


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def loaded(hiplib):
    from beifong_amd import mitsuba
    mitsuba.set_variant("scalar_rgb")
    from beifong_amd.mitsuba.core.xml import load_file
    scene = load_file(XML, spp=16)
    sensor = scene.sensors()[0]
    holder = scene.flat_desc(sensor)
    return scene, sensor, holder, capi.Scene(holder), OracleScene(holder)


def _rays(n, seed):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-3, 3, (n, 3))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(f32), d.astype(f32)


def test_ray_intersect_and_ray_test(loaded):
    scene, _, _, g, o = loaded
    orig, d = _rays(4096, 1)
    si = scene.ray_intersect(orig, d)
    rays = np.zeros((len(orig), 8), f32)
    rays[:, 0:3], rays[:, 4:7], rays[:, 7] = orig, d, np.inf
    from beifong_amd.mitsuba._host import RAY_EPSILON
    rays[:, 3] = RAY_EPSILON
    ref = g.ray_intersect(rays)
    assert np.array_equal(_bits(si.t), _bits(ref["t"])) and np.array_equal(_bits(si.p), _bits(ref["p"]))
    assert np.array_equal(_bits(si.sh_frame.n), _bits(ref["sh_n"])) and np.array_equal(_bits(si.wi), _bits(ref["wi"]))
    assert np.array_equal(_bits(si.uv), _bits(ref["prim_uv"])) and np.array_equal(_bits(si.dp_du), _bits(ref["dp_du"]))
    assert np.array_equal(si.shape, ref["shape"]) and np.array_equal(si.prim_index, ref["prim"])
    valid = si.is_valid()
    assert valid.any() and not valid.all()
    # the oracle on the same flat description: closest hits and the full record
    ot, oprim, oshape, _ = o.trace_closest(rays)
    assert np.array_equal(_bits(si.t), _bits(ot)) and np.array_equal(si.shape[valid], oshape[valid])
    for i in np.flatnonzero(valid)[:64]:
        full = o.intersect_full(rays[i])
        row = np.concatenate([[full["t"]], *[full[k] for k in ("p", "n", "sh_n", "sh_s", "sh_t", "wi", "prim_uv", "dp_du", "dp_dv")]])
        assert np.array_equal(_bits(row), _bits(ref["raw"][i])), i
    hit = scene.ray_test(rays)
    assert hit.dtype == bool and np.array_equal(hit, g.trace_any(rays).astype(bool))
    assert np.array_equal(hit, o.trace_any(rays).astype(bool))
    assert np.array_equal(scene.ray_test(orig, d), hit)


def test_shape_bsdf(loaded, hiplib):
    from tests import oracle_lib
    lib = oracle_lib.load()
    lib.bfo_material_for_side.argtypes = [C.c_void_p, C.c_uint32, C.c_float]
    lib.bfo_material_for_side.restype = C.c_uint32
    scene, _, holder, g, _ = loaded
    desc = holder.desc
    table = (capi.bf_material * desc.n_materials)(*[desc.materials[k] for k in range(desc.n_materials)])
    rng = np.random.default_rng(2)
    n = 1024
    wi = rng.normal(size=(n, 3)).astype(f32)
    wi /= np.linalg.norm(wi, axis=1, keepdims=True)
    wo = rng.normal(size=(n, 3)).astype(f32)
    wo /= np.linalg.norm(wo, axis=1, keepdims=True)
    u = rng.random((n, 3), dtype=f32)
    shapes = scene.shapes()
    assert shapes
    for sh in shapes:
        bsdf = sh.bsdf()
        k = bsdf.material
        mats = np.full(n, k, np.uint32)
        ev, pdf = bsdf.eval(wi, wo), bsdf.pdf(wi, wo)
        ref = g.bsdf_eval_pdf(mats, np.concatenate([wi, wo], 1))
        assert np.array_equal(_bits(ev), _bits(ref[:, 0])) and np.array_equal(_bits(pdf), _bits(ref[:, 1]))
        bs, w = bsdf.sample(wi, u[:, 0], u[:, 1:])
        refs = g.bsdf_sample(mats, np.concatenate([wi, u], 1))
        assert np.array_equal(_bits(bs.wo), _bits(refs[:, 0:3])) and np.array_equal(_bits(bs.pdf), _bits(refs[:, 3]))
        assert np.array_equal(_bits(w), _bits(refs[:, 4]))
        for i in range(0, n, 7):
            m = C.byref(table[lib.bfo_material_for_side(table, k, float(wi[i, 2]))])
            assert _bits(f32(lib.bfo_bsdf_eval(m, wi[i].ctypes.data, wo[i].ctypes.data))) == _bits(ev[i])
            assert _bits(f32(lib.bfo_bsdf_pdf(m, wi[i].ctypes.data, wo[i].ctypes.data))) == _bits(pdf[i])
        assert (ev > 0).any() and (w > 0).any()


def test_emitter_sample_direction(loaded):
    scene, _, holder, g, o = loaded
    ems = scene.emitters()
    assert capi.BF_EMITTER_SPOT in [e.type for e in ems]
    rng = np.random.default_rng(3)
    n = 1024
    p = rng.uniform(-2, 2, (n, 3)).astype(f32)
    s = rng.random((n, 2), dtype=f32)
    for e in ems:
        ds, spec = e.sample_direction(p, s)
        ref = g.emitter_sample_direction(e.index, np.concatenate([p, s], 1))
        assert np.array_equal(_bits(ds.d), _bits(ref[:, 0:3])) and np.array_equal(_bits(ds.pdf), _bits(ref[:, 4]))
        assert np.array_equal(_bits(ds.dist), _bits(ref[:, 3])) and np.array_equal(_bits(spec), _bits(ref[:, 6]))
        assert np.array_equal(ds.delta, ref[:, 5] != 0) and np.array_equal(_bits(ds.pdf_direction), _bits(ref[:, 7]))
        for i in range(0, n, 5):
            r = o.emitter_sample_direction(e.index, p[i], (float(s[i, 0]), float(s[i, 1])))
            assert np.array_equal(_bits(r["d"]), _bits(ds.d[i])) and _bits(f32(r["spec"])) == _bits(spec[i])
            assert _bits(f32(r["pdf"])) == _bits(ds.pdf[i]) and r["delta"] == bool(ds.delta[i])
            assert np.isclose(r["pdf_direction"], ds.pdf_direction[i], rtol=2e-6, atol=0)


def test_sensor_sample_ray(loaded):
    scene, sensor, holder, g, o = loaded
    grid = np.linspace(0, 1, 9, dtype=f32)
    pos = np.stack(np.meshgrid(grid, grid, indexing="ij"), -1).reshape(-1, 2)
    ap = np.roll(pos, 7, axis=0) * f32(0.9) + f32(0.05)
    ray, w = sensor.sample_ray(0.0, 0.5, pos, ap)
    ref = g.sensor_sample_ray(np.concatenate([pos, ap], 1).astype(f32))
    assert np.array_equal(_bits(ray.o), _bits(ref[:, 0:3])) and np.array_equal(_bits(ray.d), _bits(ref[:, 4:7]))
    assert np.array_equal(_bits(ray.mint), _bits(ref[:, 3])) and np.array_equal(_bits(w), _bits(ref[:, 7]))
    for i in range(len(pos)):
        r = o.sensor_sample_ray(float(pos[i, 0]), float(pos[i, 1]), float(ap[i, 0]), float(ap[i, 1]))
        assert np.array_equal(_bits(r["o"]), _bits(ray.o[i])) and np.array_equal(_bits(r["d"]), _bits(ray.d[i]))
        assert _bits(f32(r["weight"])) == _bits(w[i]) and _bits(f32(r["mint"])) == _bits(ray.mint[i])


TWO_SENSORS = """<scene version="2.0.0">
    <integrator type="path"/>
    <shape type="rectangle">
        <bsdf type="diffuse"/>
        <sensor type="fluxmeter"><film type="hdrfilm"><integer name="width" value="1"/><integer name="height" value="1"/></film></sensor>
    </shape>
    <shape type="rectangle">
        <transform name="to_world"><scale value="0.5"/><translate value="0, 0, 2"/></transform>
        <bsdf type="diffuse"/>
        <sensor type="fluxmeter"><film type="hdrfilm"><integer name="width" value="1"/><integer name="height" value="1"/></film></sensor>
    </shape>
    <emitter type="point"><point name="position" value="0, 0, 5"/></emitter>
    <shape type="rectangle">
        <transform name="to_world"><scale value="0.25"/><rotate x="1" angle="180"/><translate value="0.5, 0, 4"/></transform>
        <bsdf type="diffuse"/>
        <emitter type="area"><spectrum name="radiance" value="3.0"/></emitter>
    </shape>
</scene>"""


def test_each_sensor_samples_its_own_rays(hiplib):
    from beifong_amd import mitsuba
    mitsuba.set_variant("scalar_rgb")
    from beifong_amd.mitsuba.core.xml import load_string
    scene = load_string(TWO_SENSORS)
    sensors = scene.sensors()
    assert len(sensors) == 2
    pos = np.array([[0.25, 0.75], [0.5, 0.5]], f32)
    ap = np.array([[0.3, 0.6]], f32)
    rays = [s.sample_ray(0.0, 0.5, pos, ap)[0] for s in sensors]
    for s, ray in zip(sensors, rays):
        ref = OracleScene(scene.flat_desc(s))
        for i in range(len(pos)):
            r = ref.sensor_sample_ray(float(pos[i, 0]), float(pos[i, 1]), float(ap[0, 0]), float(ap[0, 1]))
            assert np.array_equal(_bits(r["o"]), _bits(ray.o[i]))
    assert not np.array_equal(rays[0].o, rays[1].o)
    assert np.allclose(rays[1].o[:, 2], 2.0)


def test_area_and_point_emitters_through_the_shim(hiplib):
    from beifong_amd import mitsuba
    mitsuba.set_variant("scalar_rgb")
    from beifong_amd.mitsuba.core.xml import load_string
    scene = load_string(TWO_SENSORS)
    ems = scene.emitters()
    assert sorted(e.type for e in ems) == sorted([capi.BF_EMITTER_POINT, capi.BF_EMITTER_AREA])
    o = OracleScene(scene.flat_desc(scene.sensors()[0]))
    rng = np.random.default_rng(5)
    p = rng.uniform(-1, 1, (64, 3)).astype(f32)
    s = rng.random((64, 2), dtype=f32)
    for e in ems:
        ds, spec = e.sample_direction(p, s)
        for i in range(64):
            r = o.emitter_sample_direction(e.index, p[i], (float(s[i, 0]), float(s[i, 1])))
            assert np.array_equal(_bits(r["d"]), _bits(ds.d[i])) and _bits(f32(r["spec"])) == _bits(spec[i])
            assert _bits(f32(r["dist"])) == _bits(ds.dist[i]) and _bits(f32(r["pdf"])) == _bits(ds.pdf[i])
            assert np.isclose(r["pdf_direction"], ds.pdf_direction[i], rtol=2e-6, atol=0)
        assert (spec > 0).any()
