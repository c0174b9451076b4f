"""Scene builders shared by the test modules (a plain module: the CPU tests use them without importing a GPU test module).

_zoo_scene: a small scene with several emitters and one-sided materials.  _fuzz_scene: random small scenes of every
integrator mode; _live_fuzz_scene: the first of its redraws whose paths carry radiance.  _bus_receive_with_mesh /
bus_radar_shifted: the C2 scenes rebuilt with the bus moved by a mesh offset (what bf_scene_translate_meshes and batched
offsets must reproduce).  oracle_rfilter: a reconstruction filter discretised by the oracle, without the host library."""
import ctypes as C

import numpy as np

from beifong_amd import capi, meshgen, scenes
from beifong_amd.scenedesc import SceneDesc, Transform4f
from tests import oracle_lib
from tests.oracle_lib import OracleScene

def _planar_uv(v):
    """Texture coordinates for the zoo meshes: an oblique planar projection, with a patch collapsed to one point so
    that some triangles carry a degenerate parameterisation (mesh.cpp:500-502 keeps coordinate_system(n) there)."""
    v = np.asarray(v, np.float32)
    uv = np.stack([0.37 * v[:, 0] + 0.11 * v[:, 2], 0.29 * v[:, 1] - 0.2 * v[:, 2]], 1).astype(np.float32)
    uv[v[:, 2] > np.quantile(v[:, 2], 0.9)] = [0.25, 0.75]
    return uv


def _zoo_scene(two_emitters=True, receive=False, uv=False):
    """Small scene exercising the branches the radar configs do not: several emitters (uniform emitter
    selection, scene.cpp:180-230 / 249-299), one-sided materials, a mesh with and a mesh without normals."""
    sd = SceneDesc()
    T = Transform4f
    d0 = T.rotate([1, 0, 0], 90) * T.rotate([0, 1, 0], 90)
    ap = T.translate([0, 0, 0.3]) * d0 * T.scale([20e-3, 50e-3, 1])
    c, lmin, lmax = sd.physics.c, sd.physics.lambda_min_nm, sd.physics.lambda_max_nm
    if receive:
        txa = sd.add_rectangle(ap, sd.add_diffuse(0.0))
        rxa = sd.add_rectangle(ap, sd.add_diffuse(0.5))
        tau = 2.0 * 0.1 / c
        f_c = c / (0.5 * (lmin + lmax) * 1e-9)
        sd.add_wigner_transmitter(txa, signaltype="pulse", amplitude=1.0, freq_centre=f_c, freq_ext=1.0 / tau, pulse_len=tau,
                                  prf=1.0 / (64 * tau), gain=1.0)
        if two_emitters:
            tx2 = sd.add_rectangle(T.translate([0.0, 1.0, 0.6]) * d0 * T.scale([0.1, 0.1, 1]), sd.add_diffuse(0.0))
            sd.add_area_transmitter(tx2, 0.5)
        sd.set_receiver(rxa, kind="omnidirectional", adc_sampling_start=0.0, adc_sampling_end=64 * tau, t_bins=64, f_bins=1,
                        t_bandwidth=64 * tau, f_bandwidth=2.0 * c / (lmin * 1e-9), freq_centre=f_c,
                        freq_ext=c / (lmin * 1e-9) - c / (lmax * 1e-9))
        lp = capi.make_launch(capi.BF_MODE_RECEIVE_RAW, 30000, seed=9, bins=64, bins_y=1)
    else:
        txa = sd.add_rectangle(ap, sd.add_diffuse(0.0))
        sd.add_area_emitter(txa, 500.0)
        if two_emitters:
            sd.add_spot(T.look_at([0.5, -1.0, 2.0], [4.0, 0.0, 0.0], [0, 0, 1]), intensity=30.0, cutoff_angle=30.0, beam_width=20.0)
            tx3 = sd.add_rectangle(T.translate([2.0, 2.0, 2.5]) * T.rotate([1, 0, 0], 180) * T.scale([0.3, 0.3, 1]), sd.add_diffuse(0.0))
            sd.add_area_emitter(tx3, 20.0)
        sd.set_perspective(T.translate([0, 0, 0.3]) * d0, fov=60.0, near_clip=0.1, far_clip=100.0)
        lp = capi.make_launch(capi.BF_MODE_RANGE, 30000, seed=9, bins=128, bin_width=0.1, color_mode=capi.BF_COLOR_RGB)
    sd.add_rectangle(T.scale([20, 20, 1]), sd.add_diffuse(0.4, twosided=False))
    v, f, n = meshgen.car_body(6000, seed=3)
    vc = meshgen.place(v, 25.0, (4.0, 0.5, 0.8))
    # uv=True: anisotropic roughness, so that the shading frame's s (from dp_du, interaction.h:159-162) shapes the lobe
    sd.add_mesh(vc, f, sd.add_roughconductor(alpha=0.3, alpha_v=0.05 if uv else None, twosided=False, specular_reflectance=0.7),
                normals=meshgen.vertex_normals(vc, f), texcoords=_planar_uv(vc) if uv else None)
    v, f = meshgen.bus(4000, seed=6)
    vb = meshgen.place(v, -40.0, (7.0, -3.0, 1.7), scale=0.5)
    sd.add_mesh(vb, f, sd.add_diffuse(0.9, twosided=True), texcoords=_planar_uv(vb) if uv else None)
    sd.finalize()
    return sd, lp


def _fuzz_receive_endpoints(sd, rng):
    """gen-3 endpoints for _fuzz_scene: one or two transmitters (wigner pulse / linfmcw, area), an omnidirectional or
    Wigner receiver with a random ADC, RECEIVE_RAW (with or without phase AOVs) or RECEIVE_IQ."""
    T = Transform4f
    c, lmin, lmax = sd.physics.c, sd.physics.lambda_min_nm, sd.physics.lambda_max_nm
    tau = float(rng.uniform(0.5, 3.0)) * 0.1 / c
    f_c = c / (0.5 * (lmin + lmax) * 1e-9)
    t_bins, f_bins = int(rng.integers(1, 96)), int(rng.choice([1, 1, 2, 5]))
    pose = T.translate([0.2, -0.3, 1.2]) * T.rotate([1, 0, 0], float(rng.uniform(100, 260))) * T.scale([0.05, 0.08, 1])
    for k in range(int(rng.integers(1, 3))):
        tx = sd.add_rectangle(pose if k == 0 else T.translate([float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)), 3.0]) *
                              T.rotate([1, 0, 0], 180) * T.scale([0.1, 0.2, 1]), sd.add_diffuse(0.0))
        if rng.random() < 0.6:
            sd.add_wigner_transmitter(tx, signaltype="linfmcw" if rng.random() < 0.4 else "pulse", amplitude=float(rng.uniform(0.5, 2)),
                                      freq_centre=f_c, freq_ext=1.0 / tau, pulse_len=tau, prf=1.0 / (t_bins * tau), gain=float(rng.uniform(0.5, 2)))
        else:
            sd.add_area_transmitter(tx, float(rng.uniform(0.5, 5)))
    rx = sd.add_rectangle(pose, sd.add_diffuse(0.5))
    sd.set_receiver(rx, kind="wigner" if rng.random() < 0.4 else "omnidirectional", adc_sampling_start=float(rng.choice([0.0, 2 * tau])),
                    adc_sampling_end=t_bins * tau, t_bins=t_bins, f_bins=f_bins, t_bandwidth=t_bins * tau,
                    f_bandwidth=2.0 * c / (lmin * 1e-9), freq_centre=f_c, freq_ext=c / (lmin * 1e-9) - c / (lmax * 1e-9),
                    gain=float(rng.uniform(0.5, 2)), sig_is_delta=bool(rng.integers(2)))
    sd.finalize()
    iq = rng.random() < 0.3
    lp = capi.make_launch(capi.BF_MODE_RECEIVE_IQ if iq else capi.BF_MODE_RECEIVE_RAW, 6000, seed=int(rng.integers(1 << 30)), bins=t_bins,
                          bins_y=f_bins, max_depth=int(rng.choice([-1, 2, 3, 8])), rr_depth=int(rng.choice([1, 3, 5, 50])),
                          phase_bins=0 if iq or rng.random() < 0.5 else int(rng.integers(1, 20)))
    return sd, lp


def _fuzz_scene(seed, receive=False):
    """A random small scene of the render modes: a box of 3-6 rectangles and 1-3 meshes with random materials
    (diffuse / rough conductor, Beckmann / GGX, one- and two-sided, isotropic or not, visible-normal sampling or
    not), a spot or area emitter (or both), fluxmeter or perspective sensor (possibly with a small film), random
    mode, colour mode, depth limits and bin widths."""
    rng = np.random.default_rng(1000 + seed + (500 if receive else 0))
    sd = SceneDesc()
    T = Transform4f

    def material():
        two = bool(rng.integers(2))
        if rng.random() < 0.45:
            return sd.add_diffuse(float(rng.uniform(0.05, 0.95)), twosided=two)
        au = float(rng.choice([0.05, 0.15, 0.4, 0.8]))
        return sd.add_roughconductor(alpha=au, alpha_v=float(rng.choice([0.05, 0.3])) if rng.random() < 0.3 else None, twosided=two,
                                     distribution="ggx" if rng.random() < 0.5 else "beckmann", sample_visible=bool(rng.integers(2)),
                                     specular_reflectance=float(rng.uniform(0.3, 1.0)) if rng.random() < 0.6 else None)

    # floor + a few random walls
    sd.add_rectangle(T.scale([6, 6, 1]), material())
    for _ in range(int(rng.integers(2, 6))):
        ax = rng.standard_normal(3)
        ax /= np.linalg.norm(ax)
        sd.add_rectangle(T.translate(list(rng.uniform(-3, 3, 2)) + [float(rng.uniform(0.3, 3))]) * T.rotate(list(ax), float(rng.uniform(0, 360))) *
                         T.scale([float(rng.uniform(0.3, 2.5)), float(rng.uniform(0.3, 2.5)), 1]), material())
    for k in range(int(rng.integers(1, 4))):
        kind = int(rng.integers(3))
        if kind == 0:
            v, f = meshgen.triangle_soup(int(rng.integers(50, 3000)), seed=seed * 7 + k, extent=1.0, size=float(rng.uniform(0.05, 0.5)))
            n = None
        elif kind == 1:
            v, f, n = meshgen.car_body(int(rng.integers(500, 4000)), seed=seed * 7 + k)
            v = v * 0.4
        else:
            v, f = meshgen.bus(int(rng.integers(500, 4000)), seed=seed * 7 + k)
            v = v * 0.25
            n = None
        v = meshgen.place(v, float(rng.uniform(0, 360)), tuple(rng.uniform(-2, 2, 2)) + (float(rng.uniform(0.5, 2.0)),))
        if kind == 1 or rng.random() < 0.4:
            n = meshgen.vertex_normals(v, f)
        sd.add_mesh(v, f, material(), normals=n, texcoords=_planar_uv(v) if rng.random() < 0.4 else None)
    if receive:
        return _fuzz_receive_endpoints(sd, rng)
    em = int(rng.integers(4))
    if em == 3:
        sd.add_point(list(rng.uniform(-3, 3, 2)) + [float(rng.uniform(1.5, 4))], intensity=float(rng.uniform(5, 50)))
        if rng.random() < 0.5:
            em = 1                                     # ... plus an area light
    if em in (0, 2):
        sd.add_spot(T.look_at(list(rng.uniform(-3, 3, 2)) + [float(rng.uniform(2, 4))], list(rng.uniform(-1, 1, 3)), [0, 0, 1]),
                    intensity=float(rng.uniform(5, 50)), cutoff_angle=float(rng.uniform(15, 60)), beam_width=float(rng.uniform(5, 14)))
    if em in (1, 2):
        r = sd.add_rectangle(T.translate([float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2)), 3.5]) * T.rotate([1, 0, 0], 180) *
                             T.scale([float(rng.uniform(0.05, 1.0)), float(rng.uniform(0.05, 1.0)), 1]), sd.add_diffuse(0.0))
        sd.add_area_emitter(r, float(rng.uniform(1, 40)))
    film, spp = None, 0
    kind = rng.random()
    if kind < 0.4:
        rx = sd.add_rectangle(T.translate([0.2, -0.3, 1.0]) * T.rotate([1, 0, 0], float(rng.uniform(90, 270))) * T.scale([0.05, 0.08, 1]),
                              sd.add_diffuse(0.5))
        if rng.random() < 0.5:
            sd.set_fluxmeter(rx)
        else:
            sd.set_irradiancemeter(rx)
    elif kind < 0.5:
        sd.set_radiancemeter(T.look_at(list(rng.uniform(-3, 3, 2)) + [float(rng.uniform(0.5, 3))], list(rng.uniform(-1, 1, 2)) + [0.5], [0, 0, 1]))
    else:
        if rng.random() < 0.5:
            film = (int(rng.integers(1, 7)), int(rng.integers(1, 5)))
        sd.set_perspective(T.look_at(list(rng.uniform(-3, 3, 2)) + [float(rng.uniform(0.5, 3))], [0, 0, 0.8], [0, 0, 1]),
                           fov=float(rng.uniform(30, 100)), near_clip=0.05, far_clip=100.0, film=film or (1, 1))
    sd.finalize()
    mode = int(rng.choice([capi.BF_MODE_PATH, capi.BF_MODE_RANGE, capi.BF_MODE_TIME]))
    n_paths = 6000
    if film:
        spp = n_paths // (film[0] * film[1])
        n_paths = spp * film[0] * film[1]
    lp = capi.make_launch(mode, n_paths, seed=int(rng.integers(1 << 30)), bins=int(rng.integers(1, 200)),
                          bin_width=float(rng.uniform(0.02, 0.5)) if mode == capi.BF_MODE_RANGE else float(rng.uniform(1e-10, 2e-9)),
                          color_mode=int(rng.integers(2)), max_depth=int(rng.choice([-1, 1, 2, 3, 8])), rr_depth=int(rng.choice([1, 3, 5, 50])),
                          film=film, spp=spp)
    return sd, lp


def _live_cells(lp, N):
    """cells a path's radiance reached: range / time bins of the films' pixels, the ADC cells' first channel (Y or I)"""
    if lp.mode in (capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ):
        c = 3 + (lp.phase_bins if lp.mode == capi.BF_MODE_RECEIVE_RAW else 0)
        return int((N.reshape(-1, c)[:, 0] >= 1).sum())
    if lp.mode in (capi.BF_MODE_RANGE, capi.BF_MODE_TIME):
        c = 5 + (lp.bins if lp.mode == capi.BF_MODE_RANGE else 3 * lp.bins)
        return int((N.reshape(-1, c)[:, 5:] >= 1).sum())
    return None


def _live_fuzz_scene(seed, receive=False):
    """The first of _fuzz_scene(seed * 1000 + j), j < 32, whose oracle render carries radiance: at least 10 % of the paths with
    a finite non-zero L and, in the range, time and receive modes, at least 3 non-base cells that some path reached.
    Returns (sd, lp, (hist, records, stats, addends)) of that render (threads=8)."""
    for j in range(32):
        sd, lp = _fuzz_scene(seed * 1000 + j, receive=receive)
        out = OracleScene(sd).render(lp, records=True, threads=8, addends=True)
        L = out[1]["L"]
        live = np.count_nonzero(np.isfinite(L) & (L != 0))
        cells = _live_cells(lp, out[3].N)
        if live >= 0.1 * lp.n_paths and (cells is None or cells >= 3):
            return sd, lp, out
    raise AssertionError(f"no live scene among the 32 draws of seed {seed} (receive={receive})")


def _bus_receive_with_mesh(v, f, t_bins=256, dr=0.1, lambda_band_nm=None):
    """scenes.bus_receive with the bus vertices replaced (same endpoints, materials, ADC)."""
    from beifong_amd import meshgen
    orig_bus, orig_place = meshgen.bus, meshgen.place
    try:
        meshgen.bus = lambda n, seed=1: (v, f)
        meshgen.place = lambda vv, yaw_deg=0.0, translate=(0, 0, 0): vv
        sd, _ = scenes.bus_receive(n_tris=len(f), n_paths=64, t_bins=t_bins, dr=dr, lambda_band_nm=lambda_band_nm)
    finally:
        meshgen.bus, meshgen.place = orig_bus, orig_place
    return sd


def bus_radar_shifted(mesh, offset, **kw):
    """scenes.bus_radar built from the placed bus mesh (scenes.bus_mesh) moved by offset: fl(p + offset), the normals kept,
    as bf_scene_translate_meshes does (test_translate_meshes_equals_rebuilt_scene)"""
    v1 = np.ascontiguousarray((mesh[0] + np.asarray(offset, np.float32)[None, :]).astype(np.float32))
    return scenes.bus_radar(mesh=(v1, mesh[1], mesh[2]), **kw)


def bus_receive_shifted(offset, n_tris=20000, **kw):
    """scenes.bus_receive(n_tris) with the placed bus moved by offset (test_batch_with_mesh_offsets_equals_translated_scenes)"""
    v, f = meshgen.bus(n_tris, seed=1)
    v = meshgen.place(v, yaw_deg=-20.0, translate=(10.0, 3.0, 1.7)).astype(np.float32)
    v1 = np.ascontiguousarray((v + np.asarray(offset, np.float32)[None, :]).astype(np.float32))
    return _bus_receive_with_mesh(v1, f, **kw)


RFILTER_KINDS = {"box": 0, "tent": 1, "gaussian": 2, "mitchell": 3, "catmullrom": 4, "lanczos": 5}


def oracle_rfilter(kind, p0=0.0, p1=0.0, block_size=0):
    """The oracle's discretisation of a reconstruction filter (which test_rfilter.py holds equal to the host plugins'
    tables), as bf_sensor.rfilter carries it"""
    lib = oracle_lib.load()
    lib.bfo_rfilter.argtypes = [C.c_int, C.c_float, C.c_float, C.POINTER(capi.bf_rfilter)]
    f = capi.bf_rfilter()
    lib.bfo_rfilter(RFILTER_KINDS[kind], p0, p1, C.byref(f))
    f.block_size = block_size
    return f
