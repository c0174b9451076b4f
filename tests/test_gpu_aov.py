"""The aov integrator (BF_FLAG_AOV): every pixel carries the AOVs of the scene's table — depth, position, uv, normals,
position partials of each path's first intersection — behind X Y Z A W, then the nested integrator's AOVs and nested.R G B A.
Expected cells come from the unchanged oracle through tests/aov_ref.py: the values from the SurfaceInteraction of every path's
composed first ray, the pixels and filter weights from every path rendered alone.  Every cell of every device histogram is held to
its per-cell fp32 summation bound; unpopulated cells are exactly zero and A, W and nested.A exact under the box filter."""
import ctypes as C
import functools

import numpy as np
import pytest

from beifong_amd import capi, motion, scenes
from beifong_amd.scenedesc import SceneDesc, Transform4f
from tests import aov_ref as ar
from tests import class_ref as cr
from tests.hist_bound import assert_fp32_sum, assert_two_fp32_sums, fp32_sum_bound
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _same_records
from tests.scene_builders import _zoo_scene, oracle_rfilter

pytestmark = pytest.mark.gpu

AOV = capi.BF_FLAG_AOV
NINE = ar.ALL_NINE
FILM_PATHS = 8 * 6 * 64
RAGGED = FILM_PATHS - 27          # no multiple of 64: the last batch of the pool is ragged


@functools.lru_cache(maxsize=None)
def _film():
    return cr.film_scene()[0]


def _film_launch(n_paths=FILM_PATHS, flags=0):
    return copy_launch(cr.film_scene()[1], n_paths=n_paths, flags=flags)


@functools.lru_cache(maxsize=None)
def _film_singles():
    return cr.single_path_hists(_film(), _film_launch())


@functools.lru_cache(maxsize=None)
def _film_expected(n_paths=FILM_PATHS, types=tuple(NINE)):
    return ar.expected(_film(), _film_launch(n_paths), list(types), singles=_film_singles())


def _against_plain(exp, h, h0, add, lp, what, sd=None):
    """base channels and nested AOVs of the AOV render against the plain render of the same handle: two fp32 sums of the same addends"""
    assert_two_fp32_sums(exp.plain_part(h), h0, add.S, add.N, what, counts=cr.count_channels(ar.plain_of(lp), sd))


def test_all_nine_types_on_the_film(hiplib):
    sd, lp = _film(), _film_launch()
    exp, rec_o, add = _film_expected()
    lay = exp.layout
    assert lay["K"] == 22 and lay["chan_px"] == 5 + 22 + 64 + 4
    assert 200 < exp.hit.sum() < FILM_PATHS - 200          # hits and misses both
    g = capi.Scene(sd)
    h0, r0, s0 = g.render(lp, records=True)
    g.set_aovs(NINE)
    assert g.channels(lp) == 48 * 69 and g.channels(ar.with_aov(lp)) == 48 * 95
    h, rec, st = g.render(ar.with_aov(lp), records=True)
    _same_records(rec, rec_o)
    _same_records(r0, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_AOV and not st.kernel_variant & capi.BF_VARIANT_LEAN and st.n_invalid == 0
    exp.check(h, "8 x 6 film, all nine types")
    _against_plain(exp, h, h0, add, lp, "all nine types against the plain render")
    img = h.reshape(6, 8, 95)
    assert np.array_equal(img[:, :, 4], np.full((6, 8), 64.0)) and np.array_equal(img[:, :, 94], img[:, :, 3])
    assert not img[:, :, lay["aovs"][7]].any() and not img[:, :, lay["aovs"][8]].any()      # duv_dx, duv_dy
    assert np.count_nonzero(img[:, :, lay["names"]["depth"]]) > 10
    # names in place of numbers, and a type twice
    g.set_aovs(["depth", "sh_normal", "depth"])
    e2, _, _ = _film_expected(types=(0, 4, 0))
    h2, _, _ = g.render(ar.with_aov(lp))
    e2.check(h2, "depth, sh_normal, depth")
    assert np.array_equal(h2.reshape(48, -1)[:, 5], h2.reshape(48, -1)[:, 9])


ROUTES = ["default", "no_tail", "small_pool", "megakernel", "global_atomics"]


def test_routes_of_one_launch(hiplib, monkeypatch):
    """The same ragged launch through every route the side rows travel: the tail's adoption of a slot, wf_shade / wf_trace to the
    end, slots that regenerate (a miss after a hit must give zeros), the one-kernel variant, global atomics."""
    exp, rec_o, _ = _film_expected(RAGGED)
    hists = {}
    for route in ROUTES:
        with monkeypatch.context() as m:
            if route == "no_tail":
                m.setenv("BF_WF_TAIL", "0")
            if route == "small_pool":
                m.setenv("BF_WF_POOL", "1024")
            g = capi.Scene(_film())
        lp = _film_launch(RAGGED, AOV | {"megakernel": capi.BF_FLAG_MEGAKERNEL, "global_atomics": capi.BF_FLAG_GLOBAL_ATOMICS}.get(route, 0))
        g.set_aovs(NINE)
        h, rec, st = g.render(lp, records=True)
        _same_records(rec, rec_o)
        assert st.kernel_variant & capi.BF_VARIANT_AOV and st.n_paths == RAGGED, route
        if route == "no_tail":
            assert st.n_bounces_tail == 0 and st.n_bounce_iters > 1
        exp.check(h, f"route {route}")
        for other, ho in hists.items():
            exp.check_two(h, ho, f"route {route} against {other}")
        hists[route] = h
        g.close()
    assert len(hists) == len(ROUTES)


def test_lds_limit(hiplib):
    """48 pixels x 256 channels = kMaxLdsHist floats fit the LDS window, 48 x 257 do not: LDS against global atomics by size"""
    sd = _film()
    g = capi.Scene(sd)
    g.set_aovs(["depth"])
    for bins, fits in ((246, True), (247, False)):
        lp = copy_launch(cr.film_scene()[1], n_paths=48 * 16, spp=16, bins=bins, bin_width=25.6 / bins)
        exp, rec_o, add = ar.expected(sd, lp, ["depth"])
        assert (g.channels(ar.with_aov(lp)) <= 12288) == fits and g.channels(ar.with_aov(lp)) == 48 * (10 + bins)
        h, rec, _ = g.render(ar.with_aov(lp), records=True)
        _same_records(rec, rec_o)
        exp.check(h, f"{bins} bins")
        hg, _, _ = g.render(ar.with_aov(lp, capi.BF_FLAG_GLOBAL_ATOMICS))
        exp.check_two(h, hg, f"{bins} bins: by size against global atomics by flag")
        _against_plain(exp, h, g.render(lp)[0], add, lp, f"{bins} bins against the plain render")


def test_time_mode_through_the_flux_meter(hiplib):
    sd, lp = scenes.trans_rad(spp=2048)
    exp, rec_o, add = ar.expected(sd, lp, NINE)
    assert 100 < exp.hit.sum() and exp.checked.size == exp.ref.size - 3      # nested.RGB: the flux meter's weight is pi
    g = capi.Scene(sd)
    g.set_aovs(NINE)
    assert g.channels(ar.with_aov(lp)) == 5 + 22 + 3 * lp.bins + 4
    h, rec, st = g.render(ar.with_aov(lp), records=True)
    _same_records(rec, rec_o)
    exp.check(h, "time mode, 1 x 1 film, flux meter")
    _against_plain(exp, h, g.render(lp)[0], add, lp, "time mode against the plain render")
    hm, _, _ = g.render(ar.with_aov(lp, capi.BF_FLAG_MEGAKERNEL))
    exp.check(hm, "time mode, one-kernel variant")
    exp.check_two(h, hm, "time mode: wavefront against the one-kernel variant")
    # nested.R = G = B, whatever it is
    rgb = h[exp.layout["nested_rgba"]]
    assert rgb[0] == rgb[1] == rgb[2] and rgb[0] != 0


def test_path_mode(hiplib):
    sd, lp = scenes.bus_radar(n_tris=2000, n_paths=2048)
    lp = copy_launch(lp, mode=capi.BF_MODE_PATH, bins=0)
    exp, rec_o, add = ar.expected(sd, lp, NINE)
    g = capi.Scene(sd)
    g.set_aovs(NINE)
    h, rec, st = g.render(ar.with_aov(lp), records=True)
    _same_records(rec, rec_o)
    assert h.size == 5 + 22 + 4 and st.kernel_variant & capi.BF_VARIANT_AOV and not st.kernel_variant & capi.BF_VARIANT_LEAN
    exp.check(h, "path mode")
    _against_plain(exp, h, g.render(lp)[0], add, lp, "path mode against the plain render")


def test_vertex_normals_and_texture_coordinates(hiplib):
    """the zoo scene of the uv-tangent parity test: a mesh with vertex normals and texture coordinates, one with texture
    coordinates alone"""
    sd, lp = _zoo_scene(uv=True)
    lp = copy_launch(lp, n_paths=2048)
    exp, rec_o, add = ar.expected(sd, lp, NINE)
    v = exp.vals[exp.hit]
    assert exp.n_tex > 300
    assert (np.abs(v[:, 6:9] - v[:, 9:12]).max(1) > 1e-3).sum() > 100           # sh_normal != geo_normal
    rays = ar.first_rays(sd, lp)
    osc = OracleScene(sd)
    prim_uv = np.array([osc.intersect_full(rays[p])["prim_uv"] for p in np.flatnonzero(exp.hit)], np.float32)
    assert (np.abs(prim_uv - v[:, 4:6]).max(1) > 1e-3).sum() > 300              # uv != prim_uv
    assert (np.abs(np.linalg.norm(v[:, 12:15], axis=1) - 1.0) > 1e-3).sum() > 100      # dp_du from the texcoords: no unit vector
    g = capi.Scene(sd)
    g.set_aovs(NINE)
    h, rec, _ = g.render(ar.with_aov(lp), records=True)
    _same_records(rec, rec_o)
    exp.check(h, "zoo scene with texture coordinates")
    hm, _, _ = g.render(ar.with_aov(lp, capi.BF_FLAG_MEGAKERNEL))
    exp.check(hm, "zoo scene with texture coordinates, one-kernel variant")
    # a rebuilt tree reorders the triangles: the texture coordinates travel with them
    g.rebuild_bvh()
    hr, rr, _ = g.render(ar.with_aov(lp), records=True)
    _same_records(rr, rec_o)
    exp.check(hr, "zoo scene after rebuild_bvh")
    _against_plain(exp, h, g.render(lp)[0], add, lp, "zoo scene against the plain render")


@pytest.mark.parametrize("case", ["gaussian", "crop", "gaussian_crop"])
def test_wide_filter_and_crop_window(hiplib, case):
    sd, lp = cr.film_scene()
    T = Transform4f
    if "crop" in case:
        d0 = T.rotate([0, 0, 1], 0.0) * T.rotate([1, 0, 0], 90) * T.rotate([0, 1, 0], 90)
        sd.set_perspective(T.translate([0.0, 0.0, 0.3]) * d0, fov=45.0, near_clip=0.1, far_clip=100.0, film=(16, 12), crop=(5, 4, 8, 6))
    if "gaussian" in case:
        sd.sensor.rfilter = oracle_rfilter("gaussian", 0.6, block_size=4)
    sd.finalize()
    lp = copy_launch(lp, n_paths=48 * 32, spp=32)
    types = ["depth", "uv", "sh_normal", "position"]
    exp, rec_o, add = ar.expected(sd, lp, types)
    assert (len(exp.counts) == 0) == ("gaussian" in case) and exp.hit.sum() > 100
    g = capi.Scene(sd)
    g.set_aovs(types)
    h, rec, st = g.render(ar.with_aov(lp), records=True)
    _same_records(rec, rec_o)
    assert bool(st.kernel_variant & capi.BF_VARIANT_WIDE) == ("gaussian" in case) and st.kernel_variant & capi.BF_VARIANT_AOV
    exp.check(h, case)
    for flag in (capi.BF_FLAG_GLOBAL_ATOMICS, capi.BF_FLAG_MEGAKERNEL):
        hf, _, _ = g.render(ar.with_aov(lp, flag))
        exp.check(hf, f"{case}, flag {flag}")
        exp.check_two(h, hf, f"{case}: default against flag {flag}")
    _against_plain(exp, h, g.render(lp)[0], add, lp, f"{case} against the plain render", sd=sd)


def _bus(n_paths=1024):
    return scenes.bus_radar(n_tris=2000, n_paths=n_paths, bins=64, dr=0.4)


def _mesh_vertices(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()


BATCH_TYPES = ["depth", "position", "geo_normal", "sh_normal", "uv"]


def test_batch_with_seeds_and_mesh_offsets(hiplib):
    sd, lp = _bus()
    seeds = [1, 31]
    offsets = np.array([[0.0, 0.0, 0.0], [0.5, -0.25, 0.125]], np.float32)
    g = capi.Scene(sd)
    g.set_aovs(BATCH_TYPES)
    hb, rb, st = g.render_batch(ar.with_aov(lp), 2, seeds=seeds, offsets=offsets, records=True)
    assert hb.shape == (2, g.channels(ar.with_aov(lp))) and st.kernel_variant & capi.BF_VARIANT_AOV
    hg, _, _ = g.render_batch(ar.with_aov(lp, capi.BF_FLAG_GLOBAL_ATOMICS), 2, seeds=seeds, offsets=offsets)
    for k in range(2):
        want = motion.deformed_description(sd, {2: (_mesh_vertices(sd, 2) + offsets[k][None, :]).astype(np.float32)})
        exp, rec_o, _ = ar.expected(want, copy_launch(lp, seed=seeds[k]), BATCH_TYPES)
        _same_records(rb[k], rec_o)
        exp.check(hb[k], f"batch render {k}")
        exp.check(hg[k], f"batch render {k}, global atomics")


def test_motion_batch(hiplib):
    sd, lp = _bus()
    xf = np.tile(motion.rigid(), (2, len(sd.shapes), 1, 1)).astype(np.float32)
    xf[1, 2] = motion.rigid(t=(1.0, -0.5, 0.0))
    g = capi.Scene(sd)
    g.set_aovs(BATCH_TYPES)
    hb, rb, st = g.render_motion_batch(ar.with_aov(lp), xf, records=True)
    assert hb.shape == (2, g.channels(ar.with_aov(lp))) and st.kernel_variant & capi.BF_VARIANT_AOV
    deps = []
    for k in range(2):
        exp, rec_o, _ = ar.expected(motion.moved_description(sd, xf[k]), lp, BATCH_TYPES)
        _same_records(rb[k], rec_o)
        exp.check(hb[k], f"motion batch render {k}")
        deps.append(exp.ref[0, 5])
    assert deps[0] != deps[1]            # the bus moved: the summed depth differs


def test_deform_batch(hiplib):
    sd, lp = _bus()
    v = _mesh_vertices(sd, 2)
    c = 0.5 * (v.min(0) + v.max(0))
    pos = np.stack([v, ((v - c) * np.array([1.0, 1.0, 1.5], np.float32) + c + np.array([0.0, -1.0, 0.0], np.float32))]).astype(np.float32)
    g = capi.Scene(sd)
    g.set_aovs(BATCH_TYPES)
    hb, rb, st = g.render_deform_batch(ar.with_aov(lp), {2: pos}, records=True)
    assert hb.shape == (2, g.channels(ar.with_aov(lp))) and st.kernel_variant & capi.BF_VARIANT_AOV
    for k in range(2):
        exp, rec_o, _ = ar.expected(motion.deformed_description(sd, {2: pos[k]}), lp, BATCH_TYPES)
        _same_records(rb[k], rec_o)
        exp.check(hb[k], f"deform batch frame {k}")


def _plate_scene(radiance=1.0, film=(5, 5), catcher=False):
    """a perspective camera at the origin looks along +x, squarely at a plate in the plane x = 5 whose normal is (-1, 0, 0); the
    matrices hold zeros and ones only, so the normal is exact.  A small lamp behind the camera lights the plate.  `catcher`: the
    lamp faces AWAY from the plate instead, towards a second plate at x = -3 behind the camera: only paths that bounce off the first
    plate onto the second one ever see the lamp."""
    sd = SceneDesc()
    M = lambda rows: Transform4f(np.array(rows + [[0, 0, 0, 1]], np.float64))
    cam = M([[0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]])
    plate = M([[0, 0, -1, 5], [0, 20, 0, 0], [20, 0, 0, 0]])
    lamp = M([[0, 0, -1, -1], [0, 0.25, 0, 0], [0.25, 0, 0, 0]]) if catcher else M([[0, 0, 1, -1], [0.25, 0, 0, 0], [0, 0.25, 0, 0]])
    sd.add_area_emitter(sd.add_rectangle(lamp, sd.add_diffuse(0.0)), radiance)
    sd.add_rectangle(plate, sd.add_diffuse(0.5, twosided=True))
    if catcher:
        sd.add_rectangle(M([[0, 0, 1, -3], [2, 0, 0, 0], [0, 2, 0, 0]]), sd.add_diffuse(0.5, twosided=True))
    sd.set_perspective(cam, fov=45.0, near_clip=0.1, far_clip=100.0, film=film)
    sd.finalize()
    return sd


def test_known_answer_plate(hiplib):
    spp = 64
    sd = _plate_scene()
    lp = capi.make_launch(capi.BF_MODE_RANGE, 25 * spp, seed=11, bins=16, bin_width=1.0, color_mode=capi.BF_COLOR_RGB, film=(5, 5), spp=spp)
    g = capi.Scene(sd)
    g.set_aovs(["sh_normal", "position", "depth", "duv_dx", "duv_dy", "geo_normal"])
    lay = capi.aov_layout(lp, ["sh_normal", "position", "depth", "duv_dx", "duv_dy", "geo_normal"])
    h, rec, _ = g.render(ar.with_aov(lp), records=True)
    img = h.reshape(5, 5, lay["chan_px"]).astype(np.float64)
    W = img[:, :, 4]
    assert np.array_equal(W, np.full((5, 5), float(spp))) and np.array_equal(img[:, :, 3], W) and (rec["valid"] == 1).all()
    for name in ("sh_normal", "geo_normal"):
        n = img[:, :, lay["names"][name]] / W[:, :, None]
        assert np.array_equal(n, np.broadcast_to(np.array([-1.0, 0.0, 0.0]), n.shape)), name
    assert not img[:, :, lay["names"]["duv_dx"]].any() and not img[:, :, lay["names"]["duv_dy"]].any()
    # position.x: 64 addends of about 5, S = 320
    b5 = float(fp32_sum_bound(5.0 * spp, spp)) / spp
    px = img[:, :, lay["names"]["position"].start] / W
    assert np.all(np.abs(px - 5.0) <= b5), (px, b5)
    # the centre pixel sees |tan| <= tan(22.5 deg) / 5 on both axes: its depths lie in 5 * [1, sqrt(1 + 2 tan^2)]
    tmax = 5.0 * np.sqrt(1.0 + 2.0 * (np.tan(np.radians(22.5)) / 5.0) ** 2)
    bd = float(fp32_sum_bound(tmax * spp, spp)) / spp
    depth = img[2, 2, lay["names"]["depth"].start] / spp
    assert 5.0 - bd <= depth <= tmax + bd, (depth, tmax, bd)
    # nested.A = A
    assert np.array_equal(img[:, :, lay["nested_rgba"].stop - 1], W)


def test_dropped_samples(hiplib):
    """A lamp of infinite radiance that the first plate cannot see: a path turns non-finite only when it bounces on to the plate
    behind the camera, vertices after its AOVs were taken, and is then dropped as a whole — its AOVs too."""
    spp = 32
    sd = _plate_scene(radiance=float("inf"), catcher=True)
    lp = capi.make_launch(capi.BF_MODE_RANGE, 25 * spp, seed=5, bins=16, bin_width=1.0, color_mode=capi.BF_COLOR_RGB, film=(5, 5), spp=spp)
    ho, ro, so = OracleScene(sd).render(lp, records=True)
    assert 0 < so.n_invalid < lp.n_paths, so.n_invalid           # the oracle drops some paths and keeps some
    assert (ro["valid"] == 1).all()                              # every path has AOV values: the dropped ones must not show
    exp, rec_o, add = ar.expected(sd, lp, NINE)
    g = capi.Scene(sd)
    g.set_aovs(NINE)
    h, rec, st = g.render(ar.with_aov(lp), records=True)
    assert st.n_invalid == so.n_invalid
    img = h.reshape(25, -1)
    assert img[:, 4].sum() == lp.n_paths - so.n_invalid
    exp.check(h, "dropped samples")
    hm, _, sm = g.render(ar.with_aov(lp, capi.BF_FLAG_MEGAKERNEL))
    assert sm.n_invalid == so.n_invalid
    exp.check(hm, "dropped samples, one-kernel variant")


def test_life_of_the_table(hiplib):
    import torch
    sd, lp = _film(), _film_launch()
    exp9, rec_o, add = _film_expected()
    exp1, _, _ = _film_expected(types=(0, 4))
    g = capi.Scene(sd)
    g.set_aovs(NINE)
    n9, n1 = 48 * 95, 48 * (5 + 4 + 64 + 4)
    # two renders on one stream with a new table between them: it takes effect for the second only
    stream = torch.cuda.Stream()
    buf = torch.zeros((2, n9), dtype=torch.float32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g.render_device(ar.with_aov(lp), buf[0].data_ptr(), stream=stream.cuda_stream)
    g.set_aovs(["depth", "sh_normal"], stream=stream.cuda_stream)
    assert g.channels(ar.with_aov(lp)) == n1
    g.render_device(ar.with_aov(lp), buf[1].data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    both = buf.cpu().numpy()
    exp9.check(both[0], "before the new table")
    exp1.check(both[1][:n1], "after the new table")
    assert not both[1][n1:].any()
    # a clone carries the table, as its own copy
    c = g.clone()
    assert c.channels(ar.with_aov(lp)) == n1
    exp1.check(c.render(ar.with_aov(lp))[0], "clone")
    c.set_aovs(NINE)
    assert g.channels(ar.with_aov(lp)) == n1
    exp1.check(g.render(ar.with_aov(lp))[0], "the original after its clone changed tables")
    c.close()
    # endpoint updates, vertex updates and rebuilds leave it alone
    g.update_endpoints(sd)
    exp1.check(g.render(ar.with_aov(lp))[0], "after update_endpoints")
    g.update_vertices(2, _mesh_vertices(sd, 2))
    g.rebuild_bvh()
    h, rec, _ = g.render(ar.with_aov(lp), records=True)
    _same_records(rec, rec_o)
    exp1.check(h, "after update_vertices and rebuild_bvh")
    # clearing it restores the plain count, and the flag has nothing to add
    g.set_aovs([])
    assert g.channels(ar.with_aov(lp)) == g.channels(lp) == 48 * 69
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_AOV.*no AOV table"):
        g.render(ar.with_aov(lp))
    assert_two_fp32_sums(g.render(lp)[0], OracleScene(sd).render(lp)[0], add.S, add.N, "plain render after clearing the table")


def _status(lib, fn, *args):
    st = fn(*args)
    return st, (lib.bf_last_error() or b"").decode()


def test_refusals(hiplib):
    import torch
    lib = hiplib
    INVALID, UNSUPPORTED = 1, capi.BF_ERR_UNSUPPORTED
    assert capi.BF_ERR_INVALID == INVALID
    sd, lp = _bus()
    g = capi.Scene(sd)
    # bf_scene_set_aovs
    for types in ([capi.BF_AOV_TYPES], [0, 99], [0] * (capi.BF_MAX_AOVS + 1)):
        a = np.asarray(types, np.uint32)
        st, msg = _status(lib, lib.bf_scene_set_aovs, g.handle, len(a), a.ctypes.data_as(C.c_void_p), None)
        assert st == INVALID and "bf_scene_set_aovs" in msg, (types, st, msg)
    g.set_aovs([4] * capi.BF_MAX_AOVS)
    assert g.channels(ar.with_aov(lp)) == 5 + 48 + 64 + 4
    g.set_aovs([])
    # the flag without a table
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_AOV.*no AOV table"):
        g.render(ar.with_aov(lp))
    g.set_aovs(NINE)
    g.set_classes([0, 0, 1], 2, 0)
    for extra, name in ((capi.BF_FLAG_FAST, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, "BF_FLAG_MOMENT"), (capi.BF_FLAG_CLASSES, "BF_FLAG_CLASSES")):
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_AOV.*{name}"):
            g.render(ar.with_aov(lp, extra))
    g.clear_classes()
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_AOV"):
        capi.render_sharded([g], ar.with_aov(lp))
    buf = torch.zeros(g.channels(ar.with_aov(lp)), dtype=torch.float32, device="cuda")
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_AOV"):
        capi.render_sharded_device([g], ar.with_aov(lp), [buf.data_ptr()])
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_AOV"):
        g.render_converge(ar.with_aov(lp), 0.1, max_rounds=2)
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_AOV"):
        g.render_converge_device(ar.with_aov(lp), buf.data_ptr(), 0.1, max_rounds=2)
    # the motion / deform batch entries refuse before they prepare anything
    xf = np.tile(motion.rigid(), (2, len(sd.shapes), 1, 1)).astype(np.float32)
    pos = np.stack([_mesh_vertices(sd, 2)] * 2)
    for extra, name in ((capi.BF_FLAG_FAST, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, "BF_FLAG_MOMENT")):
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_AOV.*{name}"):
            g.render_motion_batch(ar.with_aov(lp, extra), xf)
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_AOV.*{name}"):
            g.render_deform_batch(ar.with_aov(lp, extra), {2: pos})
    # a rolling render: refused, and the open sequence stays intact
    seq = _Sequence(g, lp, [5, 6])
    seq.issue([0])
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_AOV.*BF_FLAG_ROLLING"):
        g.render_device(ar.with_aov(lp, capi.BF_FLAG_ROLLING), buf.data_ptr())
    seq.issue([1])
    g.flush()
    h, recs = seq.results()
    assert float(buf.abs().sum()) == 0.0
    osc = OracleScene(sd)
    for k, seed in enumerate([5, 6]):
        _, ro, _, add = osc.render(copy_launch(lp, seed=seed), records=True, threads=8, addends=True)
        _same_records(recs[k], ro)
        assert_fp32_sum(h[k], add.ref, add.S, add.N, f"rolling render {k} around the refusal", counts=cr.count_channels(lp))
    # the table survived all of it
    exp, _, _ = ar.expected(sd, lp, NINE)
    exp.check(g.render(ar.with_aov(lp))[0], "after the refusals")


def test_receive_mode_is_refused(hiplib):
    sd, lp = cr.receive_scene(n_paths=256)
    g = capi.Scene(sd)
    g.set_aovs(["depth"])
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_AOV.*receive mode"):
        g.render(ar.with_aov(lp))


def test_aov_render_after_a_rolling_sequence_grew_the_pool(hiplib, monkeypatch):
    """The path pool only grows, and a rolling sequence sizes it beyond BF_WF_POOL (two renders' worth of main slots and the survivor
    area).  An AOV render of more paths than BF_WF_POOL on that handle then uses more slots than BF_WF_POOL: the side rows' stride is
    that of the pool as set up.  (A stride of BF_WF_POOL would alias the rows of different slots and run past their end.)"""
    with monkeypatch.context() as m:
        m.setenv("BF_WF_POOL", "1024")
        g = capi.Scene(_bus()[0])
    sd, lp = _bus(1024)
    seq = _Sequence(g, lp, [5, 6])
    seq.issue()
    g.flush()
    h, recs = seq.results()
    osc = OracleScene(sd)
    for k, seed in enumerate([5, 6]):
        _, ro, _, add = osc.render(copy_launch(lp, seed=seed), records=True, threads=8, addends=True)
        _same_records(recs[k], ro)
    big = copy_launch(lp, n_paths=3000 + 45)
    exp, rec_o, _ = ar.expected(sd, big, NINE)
    g.set_aovs(NINE)
    for flag in (0, capi.BF_FLAG_GLOBAL_ATOMICS):
        hb, rb, st = g.render(ar.with_aov(big, flag), records=True)
        _same_records(rb, rec_o)
        assert st.n_paths == 3045 and st.kernel_variant & capi.BF_VARIANT_AOV
        exp.check(hb, f"3045 paths after a rolling sequence under BF_WF_POOL=1024, flag {flag}")
    # ... and a small render afterwards, on the rows that render left behind
    e1, r1, _ = ar.expected(sd, lp, NINE)
    h1, rr1, _ = g.render(ar.with_aov(lp), records=True)
    _same_records(rr1, r1)
    e1.check(h1, "1024 paths afterwards")


def test_set_aovs_flushes_an_open_rolling_sequence(hiplib):
    sd, lp = _bus()
    g = capi.Scene(sd)
    seq = _Sequence(g, lp, [5])
    seq.issue([0])
    g.set_aovs(["depth"])                # the sequence ends here: its render is complete without a bf_scene_flush
    h, recs = seq.results()
    _, ro, _, add = OracleScene(sd).render(copy_launch(lp, seed=5), records=True, threads=8, addends=True)
    _same_records(recs[0], ro)
    assert_fp32_sum(h[0], add.ref, add.S, add.N, "the rolling render bf_scene_set_aovs flushed", counts=cr.count_channels(lp))
    exp, _, _ = ar.expected(sd, lp, ["depth"])
    exp.check(g.render(ar.with_aov(lp))[0], "an AOV render after the flushed sequence")


def _sequence_around(g, sd, lp, refuse, what):
    """a rolling sequence of two renders with `refuse(buf)` — the refused calls — between them: both renders are the oracle's, the
    buffer the refused calls named stays zero"""
    import torch
    buf = torch.zeros(4 * g.channels(lp) + 4096, dtype=torch.float32, device="cuda")
    seq = _Sequence(g, lp, [5, 6])
    seq.issue([0])
    refuse(buf)
    seq.issue([1])
    g.flush()
    h, recs = seq.results()
    assert float(buf.abs().sum()) == 0.0
    osc = OracleScene(sd)
    for k, seed in enumerate([5, 6]):
        _, ro, _, add = osc.render(copy_launch(lp, seed=seed), records=True, threads=8, addends=True)
        _same_records(recs[k], ro)
        assert_fp32_sum(h[k], add.ref, add.S, add.N, f"{what}: rolling render {k} around the refusals", counts=cr.count_channels(lp, sd))


def test_every_refusal_leaves_an_open_sequence_intact(hiplib):
    sd, lp = _bus()
    # no table
    g = capi.Scene(sd)

    def no_table(buf):
        with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_AOV.*no AOV table"):
            g.render_device(ar.with_aov(lp), buf.data_ptr())
    _sequence_around(g, sd, lp, no_table, "no table")
    # the flags the AOV variants do not come in, and the rolling flag itself
    g.set_classes([0, 0, 1], 2, 0)
    g.set_aovs(NINE)

    def flags(buf):
        for extra, status, name in ((capi.BF_FLAG_FAST, 1, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, 1, "BF_FLAG_MOMENT"),
                                    (capi.BF_FLAG_CLASSES, 1, "BF_FLAG_CLASSES"), (capi.BF_FLAG_ROLLING, capi.BF_ERR_UNSUPPORTED, "BF_FLAG_ROLLING")):
            with pytest.raises(capi.BeifongError, match=rf"status {status}\).*BF_FLAG_AOV.*{name}"):
                g.render_device(ar.with_aov(lp, extra), buf.data_ptr())
    _sequence_around(g, sd, lp, flags, "flags")
    exp, _, _ = ar.expected(sd, lp, NINE)
    exp.check(g.render(ar.with_aov(lp))[0], "an AOV render after the refusals")


@pytest.mark.parametrize("mode", [capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ], ids=["raw", "iq"])
def test_receive_modes_are_refused_with_a_sequence_open(hiplib, mode):
    sd, lp = cr.receive_scene(n_paths=1024)
    lp = copy_launch(lp, mode=mode)
    g = capi.Scene(sd)
    g.set_aovs(["depth", "sh_normal"])
    assert g.channels(ar.with_aov(lp)) == g.channels(lp)          # a receive launch has no AOV layout to size

    def receive(buf):
        with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_AOV.*receive mode"):
            g.render_device(ar.with_aov(lp), buf.data_ptr())
        with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_AOV.*receive mode"):
            g.render(ar.with_aov(lp))
    _sequence_around(g, sd, lp, receive, f"receive mode {mode}")
