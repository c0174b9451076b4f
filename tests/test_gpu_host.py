"""End to end through the reference-shaped surface on the GPU: XML -> host C++
plugins -> Integrator::render / receive -> C ABI -> HIP, checked against the
oracle run on the very description the host flattened."""
import os
import subprocess

import numpy as np
import pytest

from beifong_amd import capi, scenes
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.oracle_lib import OracleScene
from tests.test_host import HOST, RECEIVE_SCENE, TRANS_RAD_LIKE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mitsuba():
    from beifong_amd import mitsuba as m
    m.set_variant("scalar_rgb")
    return m


def test_render_through_the_plugin_surface(mitsuba, hiplib):
    # python_scripts/trans_rad.py:24-62 with the import changed
    from beifong_amd.mitsuba.core.xml import load_string
    scene = load_string(TRANS_RAD_LIKE, spp=20000)
    sensor = scene.sensors()[0]
    scene.integrator().render(scene, sensor)
    film = sensor.film()
    bmp = np.array(film.bitmap(raw=True))
    assert bmp.shape == (1, 1, 5 + 150) and bmp.dtype == np.float32
    names = film.bitmap(raw=True).channel_names()
    assert names[:5] == ["X", "Y", "Z", "A", "W"] and names[5] == "S0.R" and names[-1] == "S49.B"
    lp = scene.integrator().launch_for(sensor)
    ref, _, _ = OracleScene(scene.flat_desc(sensor)).render(lp, threads=8)
    assert np.allclose(bmp.reshape(-1), ref, rtol=2e-5, atol=1e-3)
    assert bmp[0, 0, 4] == 20000
    # the post-processing of trans_rad.py:46-62
    spp = sensor.sampler().sample_count()
    prof = np.array([bmp[0, 0, 5 + 3 * j:5 + 3 * j + 3].sum() / spp for j in range(50)])
    assert prof[26:28].sum() > 0 and prof[:7].sum() == 0
    st, wall_ms = scene.integrator().stats()
    assert st.n_paths == 20000 and st.n_rays_closest >= 20000


def test_receive_through_the_plugin_surface(mitsuba, hiplib):
    # Receive.ipynb cells 23-31: integrator.receive(scene, receiver); adc.bitmap(raw=True)
    from beifong_amd.mitsuba.core.xml import load_string
    mitsuba.set_variant("scalar_spectral")
    try:
        scene = load_string(RECEIVE_SCENE)
        rx = scene.receivers()[0]
        scene.integrator().receive(scene, rx)
        bmp = np.array(rx.adc().bitmap(raw=True))
        assert bmp.shape == (1, 256, 3)
        assert rx.adc().bitmap(raw=True).channel_names() == ["Y", "A", "W"]
        lp = scene.integrator().launch_for(rx)
        ref, _, _ = OracleScene(scene.flat_desc(rx)).render(lp, threads=8)
        assert np.allclose(bmp.reshape(-1), ref, rtol=2e-5, atol=1e-3)
        assert bmp[0, :, 2].sum() == 4000
    finally:
        mitsuba.set_variant("scalar_rgb")


def test_receive_mix_resample_through_the_plugin_surface(mitsuba, hiplib):
    # receive_type "mix_resample" + the integrator's Doppler switch: XML -> flags -> HIP == oracle; without the switch the
    # ADC stays empty (beat frequency 0), the reference's HEAD
    from beifong_amd.mitsuba.core.xml import load_string
    mix = RECEIVE_SCENE.replace('<receiver type="omnidirectional">',
                                '<receiver type="omnidirectional"><string name="receive_type" value="mix_resample"/>')
    dop = mix.replace('<integrator type="pathtimefrequency"/>',
                      '<integrator type="pathtimefrequency"><boolean name="doppler" value="true"/></integrator>')
    mitsuba.set_variant("scalar_spectral")
    try:
        for xml, empty in ((mix, True), (dop, False)):
            scene = load_string(xml)
            rx = scene.receivers()[0]
            scene.integrator().receive(scene, rx)
            bmp = np.array(rx.adc().bitmap(raw=True))
            lp = scene.integrator().launch_for(rx)
            ref, _, _ = OracleScene(scene.flat_desc(rx)).render(lp, threads=8)
            assert np.allclose(bmp.reshape(-1), ref, rtol=2e-5, atol=1e-3)
            assert (not bmp.any()) if empty else bmp[0, :, 2].sum() > 0
    finally:
        mitsuba.set_variant("scalar_rgb")


def test_fmcw_dechirp_through_the_plugin_surface(mitsuba, hiplib):
    # XML -> wignertransmitter resample_freq + wignerreceiver receive_type "mix_resample" (its own chirp) -> flat description ->
    # HIP == oracle: the ADC of the host object holds the de-chirped returns
    from beifong_amd.mitsuba.core.xml import load_string
    xml = RECEIVE_SCENE.replace('<string name="signaltype" value="pulse"/><float name="amplitude" value="1"/>\n'
                                '            <float name="pulse_len" value="0.000588235"/><float name="prf" value="6.640625"/>\n'
                                '            <float name="freq_centre" value="39375"/><float name="freq_ext" value="1700"/>',
                                '<string name="signaltype" value="linfmcw"/><float name="amplitude" value="1"/>'
                                '<float name="chirp_len" value="0.150588"/><float name="crf" value="6.640625"/>'
                                '<float name="freq_centre" value="39375"/><float name="freq_sweep" value="1700"/>'
                                '<boolean name="resample_freq" value="true"/>')
    xml = xml.replace('<receiver type="omnidirectional">',
                      '<receiver type="wignerreceiver"><string name="receive_type" value="mix_resample"/>'
                      '<string name="signaltype" value="linfmcw"/><float name="chirp_len" value="0.150588"/>'
                      '<float name="crf" value="6.640625"/><float name="freq_centre" value="39375"/><float name="freq_sweep" value="1700"/>')
    assert "resample_freq" in xml and "wignerreceiver" in xml
    mitsuba.set_variant("scalar_spectral")
    try:
        scene = load_string(xml)
        rx = scene.receivers()[0]
        scene.integrator().receive(scene, rx)
        bmp = np.array(rx.adc().bitmap(raw=True))
        lp = scene.integrator().launch_for(rx)
        assert lp.flags == capi.BF_FLAG_MIX_RESAMPLE
        ref, _, _ = OracleScene(scene.flat_desc(rx)).render(lp, threads=8)
        assert np.allclose(bmp.reshape(-1), ref, rtol=2e-5, atol=1e-3)
        assert bmp[0, :, 2].sum() > 0            # beats inside the ADC's 90 kHz
    finally:
        mitsuba.set_variant("scalar_rgb")


def test_bfrender_cli(hiplib, tmp_path):
    # mitsuba -m scalar_rgb -Dspp=.. scene.xml (src/mitsuba/mitsuba.cpp:173-183)
    p = tmp_path / "scene.xml"
    p.write_text(TRANS_RAD_LIKE)
    out = tmp_path / "out.npy"
    r = subprocess.run([os.path.join(HOST, "bfrender"), "-m", "scalar_rgb", "-Dspp=5000", "-o", str(out), str(p)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a = np.load(out)
    assert a.shape == (1, 1, 155) and a[0, 0, 4] == 5000
    # default output: <scene>.exr next to the scene file (mitsuba.cpp:283-290), same numbers
    r = subprocess.run([os.path.join(HOST, "bfrender"), "-m", "scalar_rgb", "-Dspp=5000", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    from beifong_amd.mitsuba import _host
    img, names = _host.read_exr(str(tmp_path / "scene.exr"))
    assert img.shape == (1, 1, 155) and sorted(names) == names and "S49.B" in names
    assert img[0, 0, names.index("W")] == 5000
    assert np.allclose(sorted(img.ravel()), sorted(a.ravel()), rtol=1e-4, atol=1e-3)
    # the long forms, a sensor index and several scene files in one call (mitsuba.cpp:171-183,228,266-292)
    p2 = tmp_path / "second.xml"
    p2.write_text(TRANS_RAD_LIKE)
    r = subprocess.run([os.path.join(HOST, "bfrender"), "--mode", "scalar_rgb", "--define", "spp=300", "--sensor", "0", "--threads", "4",
                        "--verbose", str(p), str(p2)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    for name in ("scene.exr", "second.exr"):
        img, names = _host.read_exr(str(tmp_path / name))
        assert img[0, 0, names.index("W")] == 300
    r = subprocess.run([os.path.join(HOST, "bfrender"), "-s", "3", str(p)], capture_output=True, text=True)
    assert r.returncode == 1 and "out of bounds" in r.stderr


def test_film_develop_through_the_python_layer(mitsuba, hiplib, tmp_path):
    from beifong_amd.mitsuba.core.xml import load_string
    from beifong_amd.mitsuba import _host
    scene = load_string(TRANS_RAD_LIKE, spp=2000)
    sensor = scene.sensors()[0]
    scene.integrator().render(scene, sensor)
    film = sensor.film()
    film.set_destination_file(str(tmp_path / "transient"))          # ".exr" is appended
    film.develop()
    img, names = _host.read_exr(str(tmp_path / "transient.exr"))
    bmp = film.bitmap(raw=True)
    ref = np.array(bmp)
    for k, n in enumerate(names):
        assert np.array_equal(img[:, :, k], ref[:, :, bmp.channel_names().index(n)])


FILM_SCENE = """
<scene version="2.1.0">
    <integrator type="range"><integrator type="pathlength"/><float name="dr" value="0.5"/><integer name="bins" value="20"/></integrator>
    <sensor type="perspective">
        <float name="fov" value="90"/><float name="near_clip" value="0.1"/><float name="far_clip" value="100"/>
        <transform name="to_world"><lookat origin="0, 0, 0" target="0, 0, 1" up="0, 1, 0"/></transform>
        <film type="hdrfilm"><integer name="width" value="4"/><integer name="height" value="2"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="128"/></sampler>
    </sensor>
    <shape type="rectangle">
        <transform name="to_world"><rotate y="1" angle="180"/><translate x="1" z="2"/></transform>
        <emitter type="area"><spectrum name="radiance" value="3"/></emitter>
    </shape>
</scene>
"""


def test_multi_pixel_film_through_the_plugin_surface(mitsuba, hiplib, tmp_path):
    """hdrfilm width x height > 1 x 1: sample_count paths per pixel, bitmap [H, W, 5 + bins] (integrator.cpp:58-204)."""
    from beifong_amd.mitsuba.core.xml import load_string
    scene = load_string(FILM_SCENE)
    sensor = scene.sensors()[0]
    scene.integrator().render(scene, sensor)
    bmp = np.array(sensor.film().bitmap(raw=True))
    assert bmp.shape == (2, 4, 25)
    assert np.array_equal(bmp[:, :, 4], np.full((2, 4), 128)) and np.array_equal(bmp[:, :, 3], [[128, 128, 0, 0]] * 2)
    lp = scene.integrator().launch_for(sensor)
    assert (lp.film_width, lp.film_height, lp.spp, lp.n_paths) == (4, 2, 128, 1024)
    ref, _, _ = OracleScene(scene.flat_desc(sensor)).render(lp, threads=4)
    assert np.allclose(bmp.reshape(-1), ref, rtol=2e-5, atol=1e-3)
    assert bmp[:, :2, 5:].sum() > 0 and not bmp[:, 2:, 5:].any()
    # and as an EXR of that size
    from beifong_amd.mitsuba._host import read_exr
    film = sensor.film()
    film.set_destination_file(str(tmp_path / "img"))
    film.develop()
    img, names = read_exr(str(tmp_path / "img.exr"))
    chan = film.bitmap(raw=True).channel_names()
    assert img.shape == (2, 4, 25)
    for k, n in enumerate(names):
        assert np.array_equal(img[:, :, k], bmp[:, :, chan.index(n)])


def _write_ply_be(path, v, f, normals=None):
    """binary big-endian PLY with `vertex_indices` faces (+ nx ny nz): the other byte order than this host's."""
    props = "property float x\nproperty float y\nproperty float z\n" + ("property float nx\nproperty float ny\nproperty float nz\n" if normals is not None else "")
    hdr = "ply\nformat binary_big_endian 1.0\nelement vertex %d\n%selement face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(v), props, len(f))
    rec = np.concatenate([v, normals], 1) if normals is not None else v
    with open(path, "wb") as fh:
        fh.write(hdr.encode())
        fh.write(np.ascontiguousarray(rec, ">f4").tobytes())
        fa = np.empty(len(f), dtype=[("n", "u1"), ("i", ">i4", 3)])
        fa["n"] = 3
        fa["i"] = f
        fh.write(fa.tobytes())


RADAR_MESH_SCENE = """
<scene version="2.1.0">
    <integrator type="range"><integrator type="pathlength"/><float name="dr" value="0.1"/><integer name="bins" value="256"/></integrator>
    <sensor type="perspective">
        <float name="fov" value="45"/><float name="near_clip" value="0.1"/><float name="far_clip" value="100"/>
        <transform name="to_world"><lookat origin="0, 0, 0.3" target="1, 0, 0.3" up="0, 0, 1"/></transform>
        <film type="hdrfilm"><integer name="width" value="1"/><integer name="height" value="1"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="40000"/></sampler>
    </sensor>
    <shape type="rectangle">
        <transform name="to_world"><scale x="0.02" y="0.05"/><lookat origin="0, 0, 0.3" target="1, 0, 0.3" up="0, 0, 1"/></transform>
        <emitter type="area"><spectrum name="radiance" value="1000"/></emitter>
    </shape>
    <shape type="rectangle">
        <transform name="to_world"><scale x="20" y="20"/></transform>
        <bsdf type="twosided"><bsdf type="diffuse"><spectrum name="reflectance" value="0.5"/></bsdf></bsdf>
    </shape>
    <shape type="%s">
        <string name="filename" value="%s"/>%s
        <bsdf type="twosided"><bsdf type="roughconductor"><float name="alpha" value="0.1"/></bsdf></bsdf>
    </shape>
</scene>
"""


@pytest.mark.parametrize("kind", ["obj", "ply"])
def test_file_loaded_mesh_renders_on_hip(mitsuba, hiplib, tmp_path, kind):
    """the 20 k-triangle bus written to disk — a Wavefront OBJ without `vn` lines (obj.cpp:72-354 recomputes the
    vertex normals, mesh.cpp:201-249) and a binary BIG-endian PLY carrying normals (ply.cpp:92-470) — loaded through the host
    plugins (plugins/obj.so, plugins/ply.so), rendered on HIP by Integrator::render, and compared PER PATH with the oracle run
    on the description the host flattened.  The loaded arrays equal the generator's (OBJ text round-trips fp32 through %r)."""
    from beifong_amd import meshgen
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_host import _write_obj
    v, f, n = scenes.bus_mesh(20000)
    if kind == "obj":
        _write_obj(tmp_path / "bus.obj", v, f)
        extra = ""
    else:
        _write_ply_be(tmp_path / "bus.ply", v, f, normals=n)
        extra = ""
    scene = load_string(RADAR_MESH_SCENE % (kind, "bus." + kind, extra), base_dir=str(tmp_path))
    sensor = scene.sensors()[0]
    desc = scene.flat_desc(sensor)
    sh = desc.desc.shapes[2]
    # (the generator leaves a few vertices unreferenced; the obj loader only materialises the ones faces use)
    assert sh.n_faces == len(f) and bool(sh.normals) and (sh.n_vertices == len(v) if kind == "ply" else 0 < sh.n_vertices <= len(v))
    pos = np.ctypeslib.as_array(sh.positions, shape=(sh.n_vertices, 3))
    idx = np.ctypeslib.as_array(sh.indices, shape=(sh.n_faces, 3))
    assert np.array_equal(pos[idx], v[f])        # same triangles (the obj loader numbers vertices by first use: obj.cpp:243-262)
    if kind == "ply":
        assert np.array_equal(pos, v) and np.array_equal(idx, f)
        # the loader passes normals through to_world and re-normalises them (ply.cpp:222-232): an ulp may move
        assert np.allclose(np.ctypeslib.as_array(sh.normals, shape=(len(v), 3)), n, rtol=0, atol=2e-7)
    # through the plugin surface: Integrator::render -> C ABI -> HIP
    scene.integrator().render(scene, sensor)
    bmp = np.array(sensor.film().bitmap(raw=True)).reshape(-1)
    lp = scene.integrator().launch_for(sensor)
    assert lp.n_paths == 40000 and bmp[4] == 40000
    ho, ro, so, add = OracleScene(desc).render(lp, records=True, threads=8, addends=True)
    assert np.allclose(bmp, ho, rtol=2e-5, atol=40000 * 2.0 ** -24 * max(1.0, float(np.abs(ro["L"]).max())) * 4)
    assert_fp32_sum(bmp, add.ref, add.S, add.N, "plugin surface film", counts=count_channels(lp, desc))
    assert bmp[5:].sum() > 0
    # per path, on the very description the host flattened
    g = capi.Scene(desc)
    hg, rg, sg = g.render(lp, records=True)
    for key in ("L", "aux"):
        assert np.array_equal(rg[key].view(np.uint32), ro[key].view(np.uint32))
    assert np.array_equal(rg["n_rays"], ro["n_rays"]) and np.array_equal(rg["valid"], ro["valid"])
    assert sg.n_rays_closest == so.n_rays_closest and sg.n_rays_shadow == so.n_rays_shadow
    assert sg.n_rays_traced > 1000           # rays did walk the file-loaded mesh's BVH


def test_animated_trans_rad_loop_as_the_script_writes_it(mitsuba, hiplib):
    """python_scripts/animated_trans_rad.py:100-384 with the import line changed: sampler / film / bsdf / shapes made ONCE by
    load_dict, per frame a new perspective sensor + area transmitter rectangle + scene, `scene.integrator().render(scene, sen)`
    with the load_dict'd sensor, `film.bitmap(raw=True)` on the load_dict'd film, bin j read at channel 5 + 3 j."""
    from beifong_amd.mitsuba.core.xml import load_dict
    from beifong_amd.mitsuba.core import Vector3f, Transform4f
    SPP, BINS, DR, N_FRAMES, STEP = 4000, 50, 0.2, 4, 25.0
    bsdfs = load_dict({"type": "twosided", "id": "material", "bsdf": {"type": "diffuse", "reflectance": {"type": "spectrum", "value": 1}}})
    targ = load_dict({"type": "rectangle", "id": "target", "to_world": Transform4f.look_at([0, -4, 0], [0, 0, 0], [0, 0, 1]), "bsdf": bsdfs})
    gnd = load_dict({"type": "rectangle", "id": "gnd", "to_world": Transform4f.translate([0, 0, -1]) * Transform4f.scale([10, 10, 1]), "bsdf": bsdfs})
    ints = load_dict({"type": "range", "dr": DR, "bins": BINS, "integrator": {"type": "pathlength"}})
    sampler = load_dict({"type": "independent", "sample_count": SPP})
    film = load_dict({"type": "hdrfilm", "width": 1, "height": 1, "rfilter": {"type": "box"}})
    txa_size = Transform4f.scale([0.02, 0.05, 1.0])
    rng_scan = np.zeros([N_FRAMES, BINS])
    lorigin, boresight = Vector3f(0, 0, 0), Vector3f(0, -1, 0)
    for i in range(N_FRAMES):
        rotation_cur = Transform4f.rotate(Vector3f(0, 0, 1), i * STEP)
        new_boresight_c = rotation_cur.transform_vector(boresight)
        new_up_c = rotation_cur.transform_vector(Vector3f(0, 0, 1))
        to_world_cur = Transform4f.look_at(lorigin, new_boresight_c, new_up_c)
        sen = load_dict({"type": "perspective", "near_clip": DR, "far_clip": BINS * DR + DR, "fov_axis": "x", "fov": 45,
                         "sampler": sampler, "film": film, "to_world": to_world_cur})
        emit_r = load_dict({"type": "rectangle", "id": "txa", "to_world": to_world_cur * txa_size,
                            "emitter": {"type": "area", "radiance": {"type": "spectrum", "value": 100}}})
        scene = load_dict({"type": "scene", "integrator": ints, "sensor": sen, "emitter": emit_r, "so": targ, "s1": gnd})
        scene.integrator().render(scene, sen)
        bmp22_np = np.array(film.bitmap(raw=True))
        assert bmp22_np.shape == (1, 1, 5 + BINS) and bmp22_np[0, 0, 4] == SPP
        rng_scan[i] = bmp22_np[0, 0, 5:]
    # frame 0 looks straight at the target plate 4 m away: its return sits in the bins around 2 x 4 m / 0.2 m (pathlength counts
    # the way out and back, Q1); turned 75 degrees away the plate is out of the 45-degree beam and only the ground answers
    k0 = int(np.argmax(rng_scan[0]))
    assert 36 <= k0 <= 44 and rng_scan[0, k0] > 10 * rng_scan[3, 36:45].max()
    assert sen.film().bitmap(raw=True).channel_names()[5] == "S0.Y" and sampler.sample_count() == SPP
