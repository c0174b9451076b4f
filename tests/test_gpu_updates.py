"""Endpoint updates (bf_scene_update_endpoints) for every kind of change the update accepts, under every way of issuing the
renders: material parameters, back-BSDF links, rectangle transforms, emitter records, the physics band, scenes without
rectangles, and more table versions than one rolling sequence holds.

The reference's scripts rebuild the scene for every frame (python_scripts/animated_trans_rad.py:307-384, sweep loops of
Receive.ipynb).  So every frame is held to the scene REBUILT for that frame: per-path records bit-equal to the oracle's
and to a fresh handle's stand-alone render, the histogram within the fp32 summation bound of the oracle's addends, the
weight channel equal to n_paths; and after the last flush the handle renders exactly like a fresh scene of the last frame."""
import os
import re

import numpy as np
import pytest

from beifong_amd import capi, meshgen
from beifong_amd.scenedesc import SceneDesc, Transform4f
from tests.hist_bound import assert_fp32_sum, assert_two_fp32_sums, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _launch_like, _same_records

pytestmark = pytest.mark.gpu
T = Transform4f
RECEIVE = (capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ)
N_PATHS = 1 << 13


def _roll_ring():
    """bfd::kRollRing: renders per rolling sequence and table versions per handle (bf_device.h)."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "beifong_amd", "csrc", "bf_device.h")
    with open(path) as f:
        return int(re.search(r"constexpr uint32_t kRollRing = (\d+);", f.read()).group(1))


def _mesh(n_tris=5000, seed=1):
    v, f = meshgen.bus(n_tris, seed=seed)
    v = np.ascontiguousarray(meshgen.place(v, yaw_deg=-20.0, translate=(10.0, 3.0, 1.7)), dtype=np.float32)
    f = np.ascontiguousarray(f, dtype=np.uint32)
    return v, f, np.ascontiguousarray(meshgen.vertex_normals(v, f))


def _radar(mesh, kind="range", n_paths=N_PATHS, yaw=0.0, gnd=0.5, gnd_at=(0.0, 0.0), gnd_size=20.0, car_alpha=0.1, plate_at=(3.0, -1.0, 0.6),
           back=False, emitter="area", radiance=None, band=None, bins=64, dr=0.4):
    """The bus scenes of scenes.bus_radar ("range") / scenes.bus_receive ("receive", "receive_iq") with every endpoint
    table a parameter.  A rough-conductor plate in front of the radar shows it its BACK (its normal points along +x, away
    from the radar); a spare twosided diffuse material is always in the table, so that `back` (the plate's second BSDF)
    changes no count.  Both kinds fit the lean kernel profile as long as `back` is off and the emitter is an area one."""
    sd = SceneDesc()
    c = sd.physics.c
    f_c = c / (0.5 * (sd.physics.lambda_min_nm + sd.physics.lambda_max_nm) * 1e-9)
    lmin = sd.physics.lambda_min_nm
    lmax = sd.physics.lambda_max_nm
    if band is not None:
        sd.physics.lambda_min_nm, sd.physics.lambda_max_nm = band
    pose = T.translate([0.0, 0.0, 0.3]) * T.rotate([0, 0, 1], yaw) * T.rotate([1, 0, 0], 90) * T.rotate([0, 1, 0], 90)
    aperture = pose * T.scale([20e-3, 50e-3, 1])
    txa = sd.add_rectangle(aperture, sd.add_diffuse(0.0))
    if kind == "range":
        if emitter == "area":
            sd.add_area_emitter(txa, 1000.0 if radiance is None else radiance)
        else:
            sd.add_spot(pose, intensity=1000.0 if radiance is None else radiance, cutoff_angle=30.0)
        sd.set_perspective(pose, fov=45.0, near_clip=0.1, far_clip=100.0)
    else:
        rxa = sd.add_rectangle(aperture, sd.add_diffuse(0.5))
        tau = 2.0 * dr / c
        t_total = bins * tau
        if emitter == "area":
            sd.add_area_transmitter(txa, 1.0 if radiance is None else radiance)
        else:
            sd.add_wigner_transmitter(txa, signaltype="pulse", amplitude=1.0 if radiance is None else radiance, freq_centre=f_c,
                                      freq_ext=1.0 / tau, pulse_len=tau, prf=1.0 / t_total, gain=1.0)
        sd.set_receiver(rxa, adc_sampling_start=0.0, adc_sampling_end=t_total, t_bins=bins, f_bins=1, t_bandwidth=t_total,
                        f_bandwidth=2.0 * c / (lmin * 1e-9), freq_centre=f_c, freq_ext=c / (lmin * 1e-9) - c / (lmax * 1e-9))
    sd.add_rectangle(T.translate([gnd_at[0], gnd_at[1], 0.0]) * T.scale([gnd_size, gnd_size, 1]), sd.add_diffuse(gnd, twosided=True))
    plate = sd.add_roughconductor(alpha=0.2, twosided=True, specular_reflectance=0.6)
    sd.add_rectangle(T.translate(list(plate_at)) * T.rotate([0, 1, 0], 90) * T.scale([0.8, 0.8, 1]), plate)
    spare = sd.add_diffuse(0.85, twosided=True)
    if back:
        sd.set_back_material(plate, spare)
    v, f, n = mesh
    sd.add_mesh(v, f, sd.add_roughconductor(alpha=car_alpha, twosided=True, specular_reflectance=1.0), normals=n)
    sd.finalize()
    if kind == "range":
        lp = capi.make_launch(capi.BF_MODE_RANGE, n_paths, bins=bins, bin_width=dr, color_mode=capi.BF_COLOR_RGB)
    else:
        lp = capi.make_launch(capi.BF_MODE_RECEIVE_IQ if kind == "receive_iq" else capi.BF_MODE_RECEIVE_RAW, n_paths, bins=bins,
                              bins_y=1)
    return sd, lp


def _ground_mesh(extent=20.0):
    v = np.array([[-extent, -extent, 0.0], [extent, -extent, 0.0], [extent, extent, 0.0], [-extent, extent, 0.0]], np.float32)
    return v, np.array([[0, 1, 2], [0, 2, 3]], np.uint32)


def _mesh_only(mesh, ground, n_paths=N_PATHS, pos=(0.0, 0.0, 0.3), target=(10.0, 3.0, 1.2), emitter="spot", sensor="perspective",
               radiance=1000.0, bins=64, dr=0.4):
    """A scene without rectangles: the bus and a two-triangle ground, a spot or point emitter and a 1 x 1 perspective
    sensor or a radiance meter at `pos`, looking at `target`."""
    sd = SceneDesc()
    pose = T.look_at(list(pos), list(target), [0, 0, 1])
    if emitter == "spot":
        sd.add_spot(pose, intensity=radiance, cutoff_angle=30.0)
    else:
        sd.add_point(pos, intensity=radiance)
    if sensor == "perspective":
        sd.set_perspective(pose, fov=45.0, near_clip=0.1, far_clip=100.0)
    else:
        sd.set_radiancemeter(pose)
    sd.add_mesh(ground[0], ground[1], sd.add_diffuse(0.5, twosided=True))
    v, f, n = mesh
    sd.add_mesh(v, f, sd.add_roughconductor(alpha=0.1, twosided=True, specular_reflectance=1.0), normals=n)
    sd.finalize()
    return sd, capi.make_launch(capi.BF_MODE_RANGE, n_paths, bins=bins, bin_width=dr, color_mode=capi.BF_COLOR_RGB)


def _weight(h, lp):
    """The weight channel: [4] of the render modes, the sum of column 2 (W of every ADC cell) in the receive modes."""
    if lp.mode in RECEIVE:
        return float(h.reshape(lp.bins * max(1, lp.bins_y), -1)[:, 2].sum(dtype=np.float64))
    return float(h[4])


def _check_frame(k, sd, lp, seed, h, recs, what):
    """Frame k against the scene rebuilt for it: the oracle and a fresh handle's stand-alone render."""
    l1 = _launch_like(lp, seed)
    _, ro, _, add = OracleScene(sd).render(l1, records=True, threads=8, addends=True)
    _same_records(recs, ro)
    hs, rs, _ = capi.Scene(sd).render(l1, records=True)
    _same_records(recs, rs)
    counts = count_channels(l1, sd)
    assert_fp32_sum(h, add.ref, add.S, add.N, f"{what} frame {k}", counts=counts)
    assert_two_fp32_sums(h, hs, add.S, add.N, f"{what} frame {k} vs stand-alone", counts=counts)
    assert _weight(h, lp) == lp.n_paths, (what, k, _weight(h, lp))
    return ro


ISSUE = ["plain", "rolling", "no_join", "iters1", "no_tab_cache"]


def _set_issue(issue, monkeypatch):
    """The knobs are read when a handle is created (bf_api.cpp: read_tunables)."""
    if issue == "no_join":
        monkeypatch.setenv("BF_ROLL_JOIN", "0")
    elif issue == "iters1":
        monkeypatch.setenv("BF_ROLL_ITERS", "1")
    elif issue == "no_tab_cache":
        monkeypatch.setenv("BF_TAB_CACHE", "0")


def _run(frames, issue, what, seed0=1000):
    """Render frames[k] (k > 0 after bf_scene_update_endpoints) with one handle, plain or as one rolling sequence; check
    every frame and the handle's state after the flush.  Returns (the handle, the stats of every plain render, the oracle's
    records of every frame)."""
    import torch
    sd0, lp0 = frames[0]
    g = capi.Scene(sd0)
    K, n, nch = len(frames), int(lp0.n_paths), g.channels(lp0)
    out_h, out_r, plain_st = [], [], []
    if issue == "plain":
        for k, (sd, lp) in enumerate(frames):
            if k:
                g.update_endpoints(sd)
            h, r, st = g.render(_launch_like(lp, seed0 + k), records=True)
            out_h.append(h)
            out_r.append(r)
            plain_st.append(st)
    else:
        hist = torch.zeros((K, nch), dtype=torch.float32, device="cuda")
        rec = torch.zeros((K, n, 4), dtype=torch.int32, device="cuda")
        for k, (sd, lp) in enumerate(frames):
            if k:
                g.update_endpoints(sd)
            g.render_device(_launch_like(lp, seed0 + k, flags=capi.BF_FLAG_ROLLING | capi.BF_FLAG_COUNT), hist[k].data_ptr(),
                            records_ptr=rec[k].data_ptr())
        st = g.flush(want_stats=True)
        if issue != "no_join":
            assert st.n_paths == K * n and st.n_launches_tail <= 1          # the updates joined ONE sequence
        torch.cuda.synchronize()
        out_h = list(hist.cpu().numpy())
        r = rec.cpu().numpy().view(np.uint32).reshape(K, -1, 4)
        out_r = [np.ascontiguousarray(r[k]).view(capi.PATH_RECORD_DTYPE).reshape(-1) for k in range(K)]
    oracle_recs = [_check_frame(k, sd, lp, seed0 + k, out_h[k], out_r[k], f"{what} ({issue})") for k, (sd, lp) in enumerate(frames)]
    # the handle's tables are the last frame's (home buffers again after the flush): a plain render sees them
    sdl, lpl = frames[-1]
    hl, rl, stl = g.render(_launch_like(lpl, 77), records=True)
    hf, rf, _ = capi.Scene(sdl).render(_launch_like(lpl, 77), records=True)
    _same_records(rl, rf)
    assert np.array_equal(hl[count_channels(lpl, sdl)], hf[count_channels(lpl, sdl)])
    plain_st.append(stl)
    return g, plain_st, oracle_recs


def _changed(frames, seed0=1000):
    """How many paths each update changes: the oracle's records of frame k against frame k - 1's scene at frame k's seed
    (proof that the update is seen at all, so that a kernel ignoring it could not pass)."""
    out = []
    for k in range(1, len(frames)):
        l1 = _launch_like(frames[k][1], seed0 + k)
        a = OracleScene(frames[k][0]).render(l1, records=True, threads=8)[1]
        b = OracleScene(frames[k - 1][0]).render(l1, records=True, threads=8)[1]
        out.append(int(np.count_nonzero((a["L"].view(np.uint32) != b["L"].view(np.uint32)) |
                                        (a["aux"].view(np.uint32) != b["aux"].view(np.uint32)))))
    return out


@pytest.mark.parametrize("issue", ISSUE)
@pytest.mark.parametrize("kind", ["range", "receive"])
def test_update_material_parameters(hiplib, kind, issue, monkeypatch):
    """Diffuse reflectance of the ground and alpha of the bus's rough conductor change between frames."""
    _set_issue(issue, monkeypatch)
    mesh = _mesh()
    params = [(0.5, 0.1), (0.8, 0.1), (0.8, 0.3), (0.2, 0.05)]
    frames = [_radar(mesh, kind, gnd=gd, car_alpha=a) for gd, a in params]
    _run(frames, issue, f"materials {kind}")
    assert min(_changed(frames)) > 0                 # every update changes paths


@pytest.mark.parametrize("issue", ISSUE)
@pytest.mark.parametrize("kind", ["range", "receive"])
def test_update_back_bsdf_link(hiplib, kind, issue, monkeypatch):
    """The plate's twosided material gains, loses and regains a second BSDF (the spare diffuse entry: same material count).
    Regression: bf_scene_update_endpoints kept the any_back_material bit of the scene as created, so after the link appeared
    lean_profile still chose the lean kernels, which have the back-BSDF switch compiled out: back-side hits were shaded with
    the front BSDF (records differ from the oracle's, no error)."""
    _set_issue(issue, monkeypatch)
    mesh = _mesh()
    links = [False, True, False, True]
    frames = [_radar(mesh, kind, back=b) for b in links]
    _, st, _ = _run(frames, issue, f"back BSDF {kind}")
    assert min(_changed(frames)) > 100               # paths do meet the plate from behind
    if issue == "plain":
        assert [s.kernel_variant for s in st[:len(links)]] == [capi.BF_VARIANT_LEAN if not b else 0 for b in links]
    assert st[-1].kernel_variant == 0                # the last frame has the link: general kernels


@pytest.mark.parametrize("issue", ISSUE)
@pytest.mark.parametrize("kind", ["range", "receive_iq"])
def test_update_rectangle_moves(hiplib, kind, issue, monkeypatch):
    """A non-antenna rectangle moves: the plate, then the ground (shrunk, so that it stays inside the bound the BVH boxes
    were padded for: the update refuses endpoints beyond it)."""
    _set_issue(issue, monkeypatch)
    mesh = _mesh()
    moves = [dict(), dict(plate_at=(3.0, -0.6, 0.7)), dict(plate_at=(4.0, -0.6, 0.7)), dict(plate_at=(4.0, -0.6, 0.7), gnd_at=(6.0, 6.0), gnd_size=12.0)]
    frames = [_radar(mesh, kind, **m) for m in moves]
    _run(frames, issue, f"rectangle moves {kind}")
    assert min(_changed(frames)) > 0


@pytest.mark.parametrize("issue", ISSUE)
@pytest.mark.parametrize("kind", ["range", "receive"])
def test_update_emitter_record(hiplib, kind, issue, monkeypatch):
    """The emitter's radiance changes, then its type (range: area <-> spot; receive: wigner <-> area transmitter) with the same
    emitter count: the antenna rectangle keeps its shape slot and only loses / regains its emitter index."""
    _set_issue(issue, monkeypatch)
    mesh = _mesh()
    if kind == "range":
        em = [("area", 1000.0), ("area", 250.0), ("spot", 800.0), ("area", 1000.0)]
    else:
        em = [("wigner", 1.0), ("wigner", 0.5), ("area", 1.0), ("wigner", 2.0)]
    frames = [_radar(mesh, kind, emitter=e, radiance=r) for e, r in em]
    _run(frames, issue, f"emitter {kind}")
    assert min(_changed(frames)) > 0


@pytest.mark.parametrize("issue", ISSUE)
@pytest.mark.parametrize("kind", ["receive", "receive_iq"])
def test_update_physics_band(hiplib, kind, issue, monkeypatch):
    """lambda_min / lambda_max (the wavelength every path samples) change between frames; the endpoints stay."""
    _set_issue(issue, monkeypatch)
    mesh = _mesh()
    bands = [None, (7.0e6, 9.0e6), (8.0e6, 8.2e6), (6.0e6, 1.0e7)]
    frames = [_radar(mesh, kind, band=b) for b in bands]
    _run(frames, issue, f"physics band {kind}")
    assert min(_changed(frames)) > 0


@pytest.mark.parametrize("issue", ISSUE)
@pytest.mark.parametrize("emitter,sensor", [("spot", "perspective"), ("point", "radiancemeter")])
def test_update_mesh_only_scene(hiplib, emitter, sensor, issue, monkeypatch):
    """A scene without rectangles: the radar (emitter and sensor) moves and turns between frames.  Regression: a joined
    sequence located its table block from the rectangle table's pointer, which an update of a scene without rectangles never
    moves into the pool; the flush then copied the last frame's tables from a null block."""
    _set_issue(issue, monkeypatch)
    mesh, ground = _mesh(), _ground_mesh()
    poses = [((0.0, 0.0, 0.3), (10.0, 3.0, 1.2)), ((0.5, 0.0, 0.3), (9.0, 2.0, 1.0)), ((0.5, 0.4, 0.5), (11.0, 4.0, 1.5)),
             ((1.0, -0.3, 0.3), (6.0, -1.0, 0.0))]
    frames = [_mesh_only(mesh, ground, pos=p, target=t, emitter=emitter, sensor=sensor) for p, t in poses]
    _, _, ro = _run(frames, issue, f"mesh-only {emitter}/{sensor}")
    assert all(np.count_nonzero(r["L"]) > 100 for r in ro)                     # every frame carries radiance
    assert min(_changed(frames)) > 0


def test_more_updates_than_the_ring_holds(hiplib):
    """One rolling sequence over more endpoint versions and renders than a sequence holds (bfd::kRollRing of each).  An
    update joins the open sequence while tab_next + 1 < kRollRing, else it flushes it; a render that would be render
    number kRollRing + 1 of the open sequence flushes it first.  Phase 1 updates before every render and crosses the first
    rule; phase 2 updates before every second render and crosses the second.  Every render of every frame is checked,
    and the last sequence is as long as the two rules predict."""
    import torch
    R = _roll_ring()
    n = 4096
    mesh = _mesh(5000)
    # schedule: one entry per render, the index of the endpoint version it renders with
    version = list(range(R + 2))
    while len(version) < 2 * R + 40:
        version += [version[-1] + 1] * 2
    n_versions = version[-1] + 1
    yaws = np.linspace(-25.0, 25.0, n_versions)
    frames = [_radar(mesh, "range", n_paths=n, yaw=float(y), bins=32, dr=0.8) for y in yaws]
    g = capi.Scene(frames[0][0])
    nch = g.channels(frames[0][1])
    M = len(version)
    hist = torch.zeros((M, nch), dtype=torch.float32, device="cuda")
    rec = torch.zeros((M, n, 4), dtype=torch.int32, device="cuda")
    # the host's two rules, replayed
    open_, count, tab, tails, join_flushes, render_flushes = False, 0, 0, 0, 0, 0
    for m, v in enumerate(version):
        if m and v != version[m - 1]:
            g.update_endpoints(frames[v][0])
            if open_ and tab + 1 < R:
                tab += 1
            elif open_:
                open_, count, tab, tails, join_flushes = False, 0, 0, tails + 1, join_flushes + 1
        if open_ and count + 1 > R:
            open_, count, tab, tails, render_flushes = False, 0, 0, tails + 1, render_flushes + 1
        if not open_:
            open_, count = True, 0
        count += 1
        g.render_device(_launch_like(frames[v][1], 5000 + m, flags=capi.BF_FLAG_ROLLING | capi.BF_FLAG_COUNT), hist[m].data_ptr(),
                        records_ptr=rec[m].data_ptr())
    assert (tails, join_flushes, render_flushes) == (2, 1, 1)                     # the schedule crosses both rules
    st = g.flush(want_stats=True)
    assert st.n_paths == count * n, (st.n_paths, count, tails)                    # the last sequence: as the rules predict
    torch.cuda.synchronize()
    h = hist.cpu().numpy()
    r = rec.cpu().numpy().view(np.uint32).reshape(M, -1, 4)
    cur = None
    for m, v in enumerate(version):
        sd, lp = frames[v]
        if cur is None or cur[0] != v:
            cur = (v, OracleScene(sd), capi.Scene(sd))          # the scene rebuilt for this version: oracle and a fresh handle
        l1 = _launch_like(lp, 5000 + m)
        _, ro, _, add = cur[1].render(l1, records=True, threads=16, addends=True)
        recs = np.ascontiguousarray(r[m]).view(capi.PATH_RECORD_DTYPE).reshape(-1)
        _same_records(recs, ro)
        _, rs, _ = cur[2].render(l1, records=True)
        _same_records(recs, rs)
        assert_fp32_sum(h[m], add.ref, add.S, add.N, f"ring overrun render {m} (version {v})", counts=count_channels(l1, sd))
        assert h[m][4] == n, (m, h[m][4])
    sdl, lpl = frames[-1]
    _, rl, _ = g.render(_launch_like(lpl, 77), records=True)
    _, rf, _ = capi.Scene(sdl).render(_launch_like(lpl, 77), records=True)
    _same_records(rl, rf)


def test_update_rejects_a_bad_back_material(hiplib):
    """bf_scene_update_endpoints holds the material table to what bf_scene_create does: a back_material out of range (the
    kernels would read past the device table) or pointing at an entry with a back side of its own is refused, and the
    handle keeps rendering its previous tables."""
    mesh = _mesh()
    sd0, lp = _radar(mesh)
    g = capi.Scene(sd0)
    for what in ("out of range", "names an entry with a back side"):
        sd1, _ = _radar(mesh, back=True)
        plate = next(i for i, m in enumerate(sd1.materials) if m.back_material)
        sd1.materials[plate].back_material = len(sd1.materials) + 5 if what == "out of range" else plate + 1
        sd1.finalize()
        with pytest.raises(capi.BeifongError, match="back_material"):
            g.update_endpoints(sd1)
    _, r, _ = g.render(_launch_like(lp, 3), records=True)
    _, rf, _ = capi.Scene(sd0).render(_launch_like(lp, 3), records=True)
    _same_records(r, rf)


def test_clone_while_a_joined_sequence_is_open(hiplib):
    """bf_scene_clone of a handle whose rolling sequence an endpoint update has joined: the clone ends the sequence (the last
    table version goes home), then copies the home block.  Both frames of the source are held to their rebuilt scenes, and the
    clone renders like a fresh scene of the second description.  Nothing but a flush's statistics tells whether an update
    joined, and the clone is what flushes here; so the same two frames are issued twice: the first time the flush's statistics
    show that this handle's update joins, the second time the clone ends the sequence the update joined likewise."""
    import torch
    mesh = _mesh(20000)
    frames = [_radar(mesh, "range", yaw=0.0), _radar(mesh, "range", yaw=12.0)]
    g = capi.Scene(frames[0][0])
    K, n, nch = len(frames), N_PATHS, g.channels(frames[0][1])
    hist = torch.zeros((K, nch), dtype=torch.float32, device="cuda")
    rec = torch.zeros((K, n, 4), dtype=torch.int32, device="cuda")

    def issue():
        hist.zero_()
        torch.cuda.synchronize()
        for k, (sd, lp) in enumerate(frames):
            if k:
                g.update_endpoints(sd)
            g.render_device(_launch_like(lp, 1000 + k, flags=capi.BF_FLAG_ROLLING | capi.BF_FLAG_COUNT), hist[k].data_ptr(),
                            records_ptr=rec[k].data_ptr())

    issue()
    st = g.flush(want_stats=True)
    assert st.n_paths == K * n and st.n_launches_tail <= 1          # the update joined ONE sequence
    g.update_endpoints(frames[0][0])
    issue()
    c = g.clone()
    assert g.flush(want_stats=True).n_paths == 0                    # the clone has ended the sequence
    torch.cuda.synchronize()
    h = hist.cpu().numpy()
    r = rec.cpu().numpy().view(np.uint32).reshape(K, -1, 4)
    for k, (sd, lp) in enumerate(frames):
        _check_frame(k, sd, lp, 1000 + k, h[k], np.ascontiguousarray(r[k]).view(capi.PATH_RECORD_DTYPE).reshape(-1), "clone in a joined sequence")
    sdl, lpl = frames[-1]
    _, rc, _ = c.render(_launch_like(lpl, 77), records=True)
    _, rf, _ = capi.Scene(sdl).render(_launch_like(lpl, 77), records=True)
    _same_records(rc, rf)
    _, rg, _ = g.render(_launch_like(lpl, 77), records=True)          # ... and so does the source, its tables home again
    _same_records(rg, rf)


def test_profile_follows_an_update_on_a_clone(hiplib):
    """A clone takes the source's kernel profile and an update of the clone changes the clone's alone: the clone gains a
    back-BSDF link (general kernels), the source keeps rendering with the lean ones; each matches the oracle on its own
    description."""
    mesh = _mesh(20000)
    (sd0, lp), (sd1, _) = _radar(mesh, "range"), _radar(mesh, "range", back=True)
    g = capi.Scene(sd0)
    c = g.clone()
    c.update_endpoints(sd1)
    hc, rc, stc = c.render(_launch_like(lp, 1000), records=True)
    hg, rg, stg = g.render(_launch_like(lp, 1000), records=True)
    assert stc.kernel_variant == 0 and stg.kernel_variant == capi.BF_VARIANT_LEAN
    ro0 = _check_frame(0, sd0, lp, 1000, hg, rg, "profile of the source")
    ro1 = _check_frame(1, sd1, lp, 1000, hc, rc, "profile of the clone")
    assert np.count_nonzero(ro0["L"].view(np.uint32) != ro1["L"].view(np.uint32)) > 100          # paths do meet the plate from behind
