"""The answer of a traced next-event shadow ray travels as one flag: wf_shade hands the ray to wf_trace with
kFlagShadowPending set in the stored state and occ[slot] = 0, wf_trace stores occ[slot] = 1 for an occluded ray and touches
nothing else, and whoever loads the state next (load_state: wf_shade's walks, its evicting launch, the tail's adoption of pool
slots) adds the term before anything else reads the state.  The sum is the one the reference forms (scene.cpp:220-224: an
occluded sample contributes its value times zero), so every per-path record equals the oracle's, bit for bit, through each of
those readers."""
import numpy as np
import pytest

from beifong_amd import capi, scenes
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _launch_like, _same_records, _Sequence

pytestmark = pytest.mark.gpu

N_TRIS, N_PATHS = 2000, 1 << 14


@pytest.fixture
def no_tail(monkeypatch):
    """A launch this small hands its pool to the tail kernel after the generating iteration, before wf_shade has queued one
    shadow ray.  BF_WF_TAIL=0 (read when the scene is created) keeps the tail out: wf_shade and wf_trace run every bounce."""
    monkeypatch.setenv("BF_WF_TAIL", "0")


def _same_as_oracle(rg, ro):
    for k in ("n_rays", "valid"):
        assert np.array_equal(rg[k], ro[k]), k
    for k in ("aux", "L"):
        assert np.array_equal(rg[k].view(np.uint32), ro[k].view(np.uint32)), k


@pytest.fixture(scope="module")
def range_case():
    """Case 1's scene, launch and oracle result: computed once, read by the cases that share the launch."""
    sd, lp = scenes.bus_radar(n_tris=N_TRIS, n_paths=N_PATHS, bins=256, dr=0.1)
    ho, ro, so = OracleScene(sd).render(lp, records=True, threads=8)
    return sd, lp, ro, so


def _assert_shadow_rays_of_both_kinds(sg, so):
    """The launch must exercise the flag: shadow rays exist (the oracle counts as many), wf_shade handed n_shade_shadow of
    them to wf_trace and answered the others itself, and n_rays_traced counts the handed-on ones with the closest-hit rays.
    (The statistics do not split the traced shadow rays by their answer.  The radar looks at the bus from the front: a shadow
    ray that starts on the bus and enters the root's child boxes is occluded when its vertex lies behind other geometry and
    clear when it lies on the near side; the records below hold either kind to the oracle.)"""
    assert so.n_rays_shadow > 0 and sg.n_rays_shadow == so.n_rays_shadow
    assert 0 < sg.n_shade_shadow < sg.n_rays_shadow
    assert sg.n_shade_shadow < sg.n_rays_traced <= sg.n_rays_shadow + sg.n_rays_closest


def test_range_mode_stand_alone(hiplib, range_case, no_tail):
    """Range mode, the RX = 0 kernels: every record of a launch whose shadow rays are traced, occluded or not."""
    sd, lp, ro, so = range_case
    hg, rg, sg = capi.Scene(sd).render(lp, records=True)
    assert sg.n_rays_tail == 0
    _assert_shadow_rays_of_both_kinds(sg, so)
    _same_as_oracle(rg, ro)
    assert sg.n_rays_closest == so.n_rays_closest and sg.n_invalid == so.n_invalid


def test_iq_receive(hiplib, no_tail):
    """BF_MODE_RECEIVE_IQ: the term has an imaginary part (sh3), added to the imaginary accumulator (se.w) by the same rule."""
    sd, lp = scenes.bus_receive(n_tris=N_TRIS, n_paths=N_PATHS)
    lp.mode = capi.BF_MODE_RECEIVE_IQ
    ho, ro, so = OracleScene(sd).render(lp, records=True, threads=8)
    hg, rg, sg = capi.Scene(sd).render(lp, records=True)
    assert 0 < sg.n_shade_shadow and sg.n_rays_shadow == so.n_rays_shadow and sg.n_rays_tail == 0
    assert np.count_nonzero(ro["aux"]) > 0                  # Q carries signal: the imaginary terms are not all zero
    _same_as_oracle(rg, ro)


def test_rolling_with_eviction(hiplib, monkeypatch):
    """Three rolling renders on one handle, one bounce iteration per call: the third call wakes the slots of the first
    render, whose paths of more than two vertices are still alive and move to the survivor area — a state stored with the
    flag set, and its shadow request and occ word with it, to another slot."""
    monkeypatch.setenv("BF_ROLL_ITERS", "1")
    sd, lp = scenes.bus_radar(n_tris=N_TRIS, n_paths=N_PATHS, bins=256, dr=0.1)
    g = capi.Scene(sd)
    seeds = [21, 22, 23]
    seq = _Sequence(g, lp, seeds, extra_flags=capi.BF_FLAG_STATS)
    seq.issue()
    st = g.flush(want_stats=True)
    h, recs = seq.results()
    assert st.n_guard == 0 and st.n_paths == lp.n_paths * len(seeds) and st.n_shade_shadow > 0
    o = OracleScene(sd)
    for k, seed in enumerate(seeds):
        _, ro, _ = o.render(_launch_like(lp, seed), records=True, threads=8)
        assert np.count_nonzero(ro["n_rays"] > 4) > 0       # paths that outlive two calls: the ones that move
        _same_records(recs[k], ro)


def test_tail_adopts_slots_with_a_pending_flag(hiplib, range_case, monkeypatch):
    """A pool of 4096 slots for 2^14 paths, handed to the tail once half of it is idle (BF_WF_POOL / BF_WF_TAIL, as
    test_small_pool_regenerates_paths_into_freed_slots moves the switch): the slots regenerate paths until the supply ends, so
    the switch falls in the middle of bounce iterations whose wf_shade queues shadow rays, right after a trace launch, and
    the tail adopts slots whose stored state still waits for the term of a traced shadow ray."""
    sd, lp, ro, so = range_case
    monkeypatch.setenv("BF_WF_POOL", "4096")
    monkeypatch.setenv("BF_WF_TAIL", "2048")
    g = capi.Scene(sd)
    for _ in range(2):                                      # the host-driven first render, then the planned one
        hg, rg, sg = g.render(lp, records=True)
        assert sg.n_launches_trace >= 2 and sg.n_launches_tail == 1 and sg.n_shade_shadow > 0 and sg.n_rays_tail > 0
        _same_as_oracle(rg, ro)
        assert sg.n_rays_shadow == so.n_rays_shadow


NAN_PATH = 15598114      # a path of the C2-recv scene (default seed) whose one NEE term is NaN: see _fenced_nan_scene


def _fenced_nan_scene():
    """The NaN-poison edge case (tests/test_gpu_parity.py) is a path whose receiver ray leaves IN the aperture's plane (a
    direction sample of exactly 0), lands on the coincident transmitter / receiver rectangles and samples the transmitter from
    there: an in-plane shadow ray with a NaN term, far from the mesh, so wf_shade answers it.  Arranged here so that wf_trace
    does, and finds it occluded: four small walls of the MESH stand around the sampled transmitter point X, across the
    aperture's plane, 9 mm and more from the receiver ray.  Every in-plane segment that ends at X crosses a wall, so the ray
    enters the mesh's boxes and hits a triangle.  Returns (scene, launch, rays): `rays` are shadow rays to X from every point of
    the receiver ray's line inside the aperture (the path's own among them), for the oracle to confirm the occlusion."""
    import ctypes as C
    from beifong_amd import meshgen
    from beifong_amd.scenedesc import Transform4f as T
    from tests.oracle_lib import load
    lib = load()
    u = np.zeros(8, np.float32)                   # the path's draws: fx, fy, ax, ay, time, wavelength, then the emitter sample
    lib.bfo_sampler_floats(C.c_uint64(1 + NAN_PATH), 8, u.ctypes.data_as(C.c_void_p))
    assert u[3] == 0.0                            # the direction sample that puts the receiver ray into the plane
    ap = (T.translate([0, 0, 0.3]) * T.rotate([1, 0, 0], 90) * T.rotate([0, 1, 0], 90) * T.scale([20e-3, 50e-3, 1])).matrix.astype(np.float64)
    o, X = (ap @ [u[0] * 2 - 1, u[1] * 2 - 1, 0, 1])[:3], (ap @ [u[6] * 2 - 1, u[7] * 2 - 1, 0, 1])[:3]
    r, h, vs, fs = 2e-3, 1.5e-3, [], []           # walls: the sides of the square of half-width r around X, half a side longer
    for c, w in (((0, r, 0), (0, 0, 1.5 * r)), ((0, -r, 0), (0, 0, 1.5 * r)), ((0, 0, r), (0, 1.5 * r, 0)), ((0, 0, -r), (0, 1.5 * r, 0))):
        c, w, n, k = X + np.array(c), np.array(w), np.array([h, 0.0, 0.0]), len(vs)
        vs += [c - w - n, c + w - n, c + w + n, c - w + n]
        fs += [[k, k + 1, k + 2], [k, k + 2, k + 3]]
    v, f = meshgen.bus(N_TRIS, seed=1)
    a = np.radians(-20.0)                         # bus_receive places the whole mesh (yaw -20 degrees, then the shift): undone for the walls
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    walls = (np.array(vs) - np.array([10.0, 3.0, 1.7])) @ rot
    mesh = (np.concatenate([v.astype(np.float64), walls]).astype(np.float32), np.concatenate([f, np.array(fs, np.uint32) + len(v)]).astype(np.uint32))
    sd, lp = scenes.bus_receive(n_tris=N_TRIS, n_paths=1, mesh=mesh)
    lp.path_offset = NAN_PATH
    # the receiver ray's in-plane direction: the cosine-hemisphere sample (ax, 0) in the frame of the aperture's normal
    loc, nn, sv, tv = np.zeros(3, np.float32), np.ascontiguousarray(ap[:3, 2] / np.linalg.norm(ap[:3, 2]), np.float32), np.zeros(3, np.float32), np.zeros(3, np.float32)
    lib.bfo_square_to_cosine_hemisphere(C.c_float(u[2]), C.c_float(u[3]), loc.ctypes.data_as(C.c_void_p))
    lib.bfo_coordinate_system(nn.ctypes.data_as(C.c_void_p), sv.ctypes.data_as(C.c_void_p), tv.ctypes.data_as(C.c_void_p))
    d = sv * loc[0] + tv * loc[1] + nn * loc[2]
    P = o[None, :] + np.linspace(1e-3, 0.12, 400)[:, None] * d[None, :]
    P = P[(np.abs(P[:, 1]) <= 0.02) & (np.abs(P[:, 2] - 0.3) <= 0.05)]
    to_x = X[None, :] - P
    dist = np.linalg.norm(to_x, axis=1)
    assert len(P) > 50 and dist.min() > 4 * r     # the receiver ray passes well outside the walls
    rays = np.concatenate([P, np.full((len(P), 1), 1e-4), to_x / dist[:, None], (dist * (1 - 1e-3))[:, None]], axis=1)
    return sd, lp, rays


@pytest.mark.parametrize("iq", [False, True])
def test_non_finite_term_of_a_traced_occluded_ray_survives(hiplib, no_tail, iq):
    """One path, tail off.  Oracle side first: the path's radiance is NaN, it has one shadow ray, and that ray is occluded
    wherever on its line the receiver ray ended.  Device: wf_shade hands that one ray to wf_trace (n_shade_shadow == 1), which
    stores occ = 1; load_state adds NaN * 0, and the record is the oracle's NaN — in I/Q mode both accumulators'."""
    sd, lp, rays = _fenced_nan_scene()
    if iq:
        lp.mode = capi.BF_MODE_RECEIVE_IQ
    o = OracleScene(sd)
    ho, ro, so = o.render(lp, records=True)
    assert np.isnan(ro["L"][0]) and so.n_invalid == 1 and so.n_rays_shadow == 1 and (np.isnan(ro["aux"][0]) or not iq)
    assert o.trace_any(rays).all()
    hg, rg, sg = capi.Scene(sd).render(lp, records=True)
    assert sg.n_rays_tail == 0 and sg.n_shade_shadow == 1 and sg.n_rays_shadow == 1
    assert np.array_equal(rg.view(np.uint32), ro.view(np.uint32)) and sg.n_invalid == 1


def test_lean_against_general(hiplib, range_case, no_tail, monkeypatch):
    """BF_LEAN=0 (read when the scene is created) forces the general shading kernels on case 1: same records from both,
    and both the oracle's."""
    sd, lp, ro, so = range_case
    out = {}
    for lean in ("1", "0"):
        monkeypatch.setenv("BF_LEAN", lean)
        hg, rg, sg = capi.Scene(sd).render(lp, records=True)
        assert sg.kernel_variant == (capi.BF_VARIANT_LEAN if lean == "1" else 0) and sg.n_shade_shadow > 0
        _same_as_oracle(rg, ro)
        out[lean] = (rg, sg)
    assert np.array_equal(out["1"][0], out["0"][0])
    assert out["1"][1].n_shade_shadow == out["0"][1].n_shade_shadow and out["1"][1].n_rays_traced == out["0"][1].n_rays_traced
