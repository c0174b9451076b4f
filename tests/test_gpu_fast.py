"""BF_FLAG_FAST: the kernels' fast-arithmetic build (approximate fp32 division and square root, include/beifong_hip.h).

Fast renders are held to the tolerance contract of tests/fast_contract.py against the oracle, to bit-equality among
themselves whatever launch runs them, and must not leak into the exact renders of the same handle."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from beifong_amd import capi, scenes
from beifong_amd.scenedesc import Transform4f
from tests import fast_contract as fc
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _launch_like, _same_records, _Sequence
from tests.scene_builders import _live_fuzz_scene, _zoo_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST = capi.BF_FLAG_FAST

# Share of paths that do not agree with the oracle's (fast_contract.agreement), per scene: pinned on an MI355X at no more than
# twice the measured share (fast renders are deterministic), never above the contract's hard cap of 1 %.
CAP = 0.01
DIVERGED_PIN = {            # measured on an MI355X: diverged paths / paths (the wavefront and one-kernel pipelines agree)
    "bus_radar": 2 * 266 / 65536,
    "bus_receive_wigner": 0.0,
    "bus_receive_area": 0.0,
    "plate_doppler_iq": 2 * 96 / 65536,
    "fmcw_plate_mix": 0.0,
    "two_bsdf": 2 * 5 / 30000,
    "film_range": 0.0,
    "fuzz0": 2 * 1 / 6000,
    "fuzz1": 2 * 6 / 6000,
    "fuzz2": 0.0,
    "fuzz3": 2 * 2 / 6000,
    "fuzz4": 2 * 5 / 6000,
    "fuzz5": 0.0,
    "fuzz6": 0.0,
    "fuzz7": 2 * 10 / 6000,
}


def _pin(name):
    return min(DIVERGED_PIN[name], CAP)


def _w_channels(lp):
    """flat indices of the weight channel W of every pixel / ADC cell"""
    if lp.mode in (capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ):
        c = 3 + (lp.phase_bins if lp.mode == capi.BF_MODE_RECEIVE_RAW else 0)
        return np.arange(lp.bins * max(lp.bins_y, 1), dtype=np.int64) * c + 2
    c = {capi.BF_MODE_PATH: 5, capi.BF_MODE_RANGE: 5 + lp.bins, capi.BF_MODE_TIME: 5 + 3 * lp.bins}[lp.mode]
    px = lp.film_width * lp.film_height if (lp.spp and lp.film_width and lp.film_height) else 1
    return np.arange(px, dtype=np.int64) * c + 4


def _contract(name, sd, lp, pipelines=(0,), oracle_out=None, g=None):
    """Render `lp` fast on every pipeline (extra flags) and hold each result to the contract; returns the fast records"""
    base = lp.flags & ~FAST
    lp.flags = base
    ho, ro, so, add = oracle_out if oracle_out is not None else OracleScene(sd).render(lp, records=True, threads=16, addends=True)
    g = g or capi.Scene(sd)
    exact_film = fc.is_box_1x1(sd, lp) and sd.desc.sensor.type == capi.BF_SENSOR_PERSPECTIVE
    if exact_film:
        # item 2: the restated rule must give the oracle's own histogram from the oracle's records
        ref, S, N = fc.film_addends(ro, lp)
        assert np.array_equal(N, np.asarray(add.N).reshape(-1).astype(np.int64)), f"{name}: restated binning rule, counts"
        Sa = np.asarray(add.S, np.float64).reshape(-1)
        assert np.all(np.abs(ref - np.asarray(add.ref).reshape(-1)) <= 1e-12 * Sa), f"{name}: restated binning rule, sums"
        assert np.allclose(S, Sa, rtol=1e-12, atol=0), f"{name}: restated binning rule, magnitudes"
    out = None
    for extra in pipelines:
        lp.flags = base | extra | FAST
        hf, rf, sf = g.render(lp, records=True)
        lp.flags = base
        what = f"{name} flags {extra:#x}"
        assert sf.kernel_variant & capi.BF_VARIANT_FAST, what
        assert sf.n_paths == lp.n_paths, what
        agree, worst = fc.agreement(rf, ro)
        diverged = 1.0 - float(agree.mean())
        figs = dict(scene=name, flags=extra, n_paths=int(lp.n_paths), diverged=diverged, n_diverged=int((~agree).sum()),
                    max_rel_dL=worst, rmse=fc.rmse(hf, ho), bitwise_differ=int((rf["L"].view(np.uint32) != ro["L"].view(np.uint32)).sum()))
        wch = _w_channels(lp)
        if len(count_channels(lp, sd)):
            assert float(hf[wch].astype(np.float64).sum()) == float(ho[wch].astype(np.float64).sum()), f"{what}: total weight"
        if exact_film:
            ref, S, N = fc.film_addends(rf, lp)
            figs["cell_ratio"] = assert_fp32_sum(hf, ref, S, N, f"{what}: fast histogram vs its own records", counts=count_channels(lp, sd))
            fc.log(**figs)
        else:
            err, bound, n_edge = fc.whole_hist_bound(hf, ho, add, rf, ro, agree, sd, lp)
            figs.update(hist_err=err, hist_bound=bound, n_edge=n_edge)
            fc.log(**figs)
            assert err <= bound, f"{what}: sum |h_F - h_O| = {err:.6g} above the bound {bound:.6g}"
        assert diverged <= _pin(name), f"{what}: {figs['n_diverged']} of {lp.n_paths} paths diverged ({diverged:.3%})"
        out = rf
    return out


def _two_bsdf_scene():
    T = Transform4f
    sd, lp = _zoo_scene(two_emitters=True)
    front = sd.add_roughconductor(alpha=0.2, twosided=True, specular_reflectance=0.6)
    sd.add_rectangle(T.translate([2.0, -0.2, 0.9]) * T.rotate([0, 1, 0], 90) * T.scale([1.0, 1.2, 1]), front)
    sd.set_back_material(front, sd.add_diffuse(reflectance=0.85, twosided=True))
    for i in range(len(sd.materials)):
        if sd.materials[i].type == capi.BF_BSDF_ROUGHCONDUCTOR and i != front:
            sd.set_back_material(i, sd.add_diffuse(reflectance=0.3, twosided=True))
    sd.finalize()
    return sd, lp


def _scene(name):
    if name == "bus_radar":
        return scenes.bus_radar(n_paths=1 << 16)
    if name in ("bus_receive_wigner", "bus_receive_area"):
        return scenes.bus_receive(n_paths=1 << 16, transmitter=name.rsplit("_", 1)[1])
    if name == "plate_doppler_iq":
        return scenes.plate_doppler(n_paths=1 << 16)
    if name == "fmcw_plate_mix":
        return scenes.fmcw_plate(n_paths=1 << 18)
    if name == "two_bsdf":
        return _two_bsdf_scene()
    if name == "film_range":
        return scenes.film_half_lit(film=(8, 4), spp=512, mode=capi.BF_MODE_RANGE, bins=32, dr=0.25)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["bus_radar", "bus_receive_wigner", "bus_receive_area", "plate_doppler_iq", "fmcw_plate_mix",
                                  "two_bsdf", "film_range"])
def test_fast_contract(hiplib, name):
    sd, lp = _scene(name)
    rf = _contract(name, sd, lp, pipelines=(0,) if name != "two_bsdf" else (0, capi.BF_FLAG_MEGAKERNEL))
    if name == "bus_radar":
        # the fast kernels really ran: their records are not the exact ones
        lp.flags = 0
        _, re_, se = capi.Scene(sd).render(lp, records=True)
        assert not (se.kernel_variant & capi.BF_VARIANT_FAST)
        assert np.any(rf["L"].view(np.uint32) != re_["L"].view(np.uint32))


@pytest.mark.parametrize("seed", range(8))
def test_fast_contract_live_fuzz(hiplib, seed):
    sd, lp, out = _live_fuzz_scene(seed)
    _contract(f"fuzz{seed}", sd, lp, pipelines=(0, capi.BF_FLAG_MEGAKERNEL), oracle_out=out)


def _child_records(sd_builder, lp_args, env, tmp_path):
    """records of one fast render in a fresh process (BF_* knobs are read when a scene is created)"""
    out = tmp_path / "rec.npy"
    code = (f"import sys; sys.path.insert(0, {ROOT!r})\n"
            "import numpy as np\n"
            "from beifong_amd import capi, scenes\n"
            f"sd, lp = scenes.{sd_builder}\n"
            f"lp.flags = {lp_args}\n"
            "h, r, st = capi.Scene(sd).render(lp, records=True)\n"
            f"np.save({str(out)!r}, r)\n"
            "print(st.kernel_variant)\n")
    p = subprocess.run([sys.executable, "-c", code], env={**os.environ, **env}, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    return np.load(out), int(p.stdout.split()[-1])


def test_fast_records_identical_across_launches(hiplib, tmp_path):
    """A fast path is the same path whatever launch runs it: stand-alone twice, a flushed rolling sequence of four, a seeded
    batch of four, the one-kernel variant, the general kernels (BF_LEAN=0, fresh process), a one-device sharded render and a
    rolling sequence joined across endpoint updates."""
    import torch
    n = 1 << 16
    mesh = scenes.bus_mesh(20000)
    sd, lp = scenes.bus_radar(n_paths=n, bins=256, dr=0.1, mesh=mesh)
    g = capi.Scene(sd)
    seeds = [21, 22, 23, 24]
    ref = {}
    for s in seeds:
        h1, r1, s1 = g.render(_launch_like(lp, s, flags=FAST), records=True)
        h2, r2, s2 = g.render(_launch_like(lp, s, flags=FAST), records=True)
        _same_records(r1, r2)
        assert s1.kernel_variant == capi.BF_VARIANT_LEAN | capi.BF_VARIANT_FAST
        ref[s] = r1
    # rolling sequence of four, flushed
    seq = _Sequence(g, _launch_like(lp, 0, flags=FAST), seeds)
    seq.issue()
    st = g.flush(want_stats=True)
    assert st.kernel_variant & capi.BF_VARIANT_FAST
    h, recs = seq.results()
    for k, s in enumerate(seeds):
        _same_records(recs[k], ref[s])
        assert float(h[k][4]) == float(n)
    # seeded batch of four
    hb, rb, sb = g.render_batch(_launch_like(lp, 0, flags=FAST), 4, seeds=seeds, records=True)
    assert sb.kernel_variant & capi.BF_VARIANT_FAST
    for k, s in enumerate(seeds):
        _same_records(rb[k], ref[s])
    # the one-kernel variant
    _, rm, sm = g.render(_launch_like(lp, seeds[0], flags=FAST | capi.BF_FLAG_MEGAKERNEL), records=True)
    assert sm.kernel_variant == capi.BF_VARIANT_FAST
    _same_records(rm, ref[seeds[0]])
    # the general kernels, in a fresh process
    rgen, var = _child_records("bus_radar(n_paths=%d, bins=256, dr=0.1, mesh=scenes.bus_mesh(20000))" % n,
                               "capi.BF_FLAG_FAST; lp.seed = %d" % seeds[1], {"BF_LEAN": "0"}, tmp_path)
    assert var == capi.BF_VARIANT_FAST
    _same_records(rgen, ref[seeds[1]])
    # a one-device sharded render (no records): its histogram is the fp32 sum of the stand-alone fast render's records
    d = torch.zeros(g.channels(lp), dtype=torch.float32, device="cuda")
    capi.render_sharded_device([g], _launch_like(lp, seeds[2], flags=FAST), [d.data_ptr()])
    torch.cuda.synchronize()
    l2 = _launch_like(lp, seeds[2])
    ref_, S_, N_ = fc.film_addends(ref[seeds[2]], l2)
    assert_fp32_sum(d.cpu().numpy(), ref_, S_, N_, "one-device sharded fast render", counts=count_channels(l2, sd))
    # a rolling sequence joined across endpoint updates: the paths of every frame are that frame's stand-alone fast paths
    yaws = [0.0, 6.0, -9.0]
    frames = [scenes.bus_radar(n_paths=n, bins=256, dr=0.1, radar_yaw_deg=y, mesh=mesh) for y in yaws]
    gj = capi.Scene(frames[0][0])
    hist = torch.zeros((len(frames), gj.channels(lp)), dtype=torch.float32, device="cuda")
    rec = torch.zeros((len(frames), n, 4), dtype=torch.int32, device="cuda")
    for k, (sdk, lpk) in enumerate(frames):
        if k:
            gj.update_endpoints(sdk)
        gj.render_device(_launch_like(lpk, 500 + k, flags=capi.BF_FLAG_ROLLING | capi.BF_FLAG_COUNT | FAST), hist[k].data_ptr(),
                         records_ptr=rec[k].data_ptr())
    st = gj.flush(want_stats=True)
    assert st.n_paths == len(frames) * n and st.kernel_variant & capi.BF_VARIANT_FAST
    torch.cuda.synchronize()
    r = rec.cpu().numpy().view(np.uint32).reshape(len(frames), -1, 4)
    for k, (sdk, lpk) in enumerate(frames):
        recs_k = np.ascontiguousarray(r[k]).view(capi.PATH_RECORD_DTYPE).reshape(-1)
        _, rs, _ = capi.Scene(sdk).render(_launch_like(lpk, 500 + k, flags=FAST), records=True)
        _same_records(recs_k, rs)


def test_no_leak_between_modes(hiplib):
    """exact, fast, exact on one handle: both exact renders are the oracle's, bit for bit, and carry no fast bit"""
    sd, lp = scenes.bus_radar(n_tris=20000, n_paths=1 << 15, bins=256, dr=0.1)
    _, ro, _ = OracleScene(sd).render(lp, records=True, threads=16)
    g = capi.Scene(sd)
    seen = []
    for flags in (0, FAST, 0):
        lp.flags = flags
        _, r, s = g.render(lp, records=True)
        assert bool(s.kernel_variant & capi.BF_VARIANT_FAST) == bool(flags)
        seen.append(r)
    _same_records(seen[0], ro)
    _same_records(seen[2], ro)
    assert np.any(seen[1]["L"].view(np.uint32) != ro["L"].view(np.uint32))
    # and a fast rolling sequence between exact ones: the flush of each runs its own mode's kernels
    for flags in (0, FAST, 0):
        seq = _Sequence(g, _launch_like(lp, 3, flags=flags), [3, 4])
        seq.issue()
        g.flush()
        _, recs = seq.results()
        _, rs, _ = g.render(_launch_like(lp, 4, flags=flags), records=True)
        _same_records(recs[1], rs)


@pytest.mark.parametrize("open_fast", [False, True])
def test_mixing_modes_in_a_rolling_sequence_is_an_error(hiplib, open_fast):
    """A rolling render whose BF_FLAG_FAST differs from the open sequence's fails before anything is enqueued; the sequence
    stays intact: its flush completes every path it holds."""
    import torch
    n = 1 << 15
    sd, lp = scenes.bus_radar(n_tris=20000, n_paths=n, bins=256, dr=0.1)
    g = capi.Scene(sd)
    mode = FAST if open_fast else 0
    seq = _Sequence(g, _launch_like(lp, 0, flags=mode), [7, 8])
    seq.issue()
    other = torch.zeros(g.channels(lp), dtype=torch.float32, device="cuda")
    bad = _launch_like(lp, 9, flags=capi.BF_FLAG_ROLLING | (mode ^ FAST))
    status = hiplib.bf_render_device(g.handle, C.byref(bad), C.c_void_p(other.data_ptr()), None, None, None)
    assert status == capi.BF_ERR_INVALID and "BF_FLAG_FAST" in hiplib.bf_last_error().decode()
    st = g.flush(want_stats=True)
    assert st.n_paths == 2 * n and bool(st.kernel_variant & capi.BF_VARIANT_FAST) == open_fast
    h, recs = seq.results()
    assert [float(hk[4]) for hk in h] == [float(n)] * 2
    assert not other.cpu().numpy().any()
    for k, s in enumerate((7, 8)):
        _, rs, _ = g.render(_launch_like(lp, s, flags=mode), records=True)
        _same_records(recs[k], rs)


def _host_contract(what, desc, lp, h_fast):
    """a fast film from the host layer against the contract: the records are those of the same fast launch through the C ABI"""
    lp.flags &= ~FAST
    ho, ro, so, add = OracleScene(desc).render(lp, records=True, threads=16, addends=True)
    lp.flags |= FAST
    _, rf, sf = capi.Scene(desc).render(lp, records=True)
    lp.flags &= ~FAST
    agree, worst = fc.agreement(rf, ro)
    err, bound, n_edge = fc.whole_hist_bound(h_fast, ho, add, rf, ro, agree, desc, lp)
    fc.log(scene=what, diverged=1.0 - float(agree.mean()), max_rel_dL=worst, rmse=fc.rmse(h_fast, ho), hist_err=err, hist_bound=bound)
    assert err <= bound, f"{what}: sum |h_F - h_O| = {err:.6g} above the bound {bound:.6g}"
    wch = _w_channels(lp)
    assert float(np.asarray(h_fast, np.float64).reshape(-1)[wch].sum()) == float(ho[wch].astype(np.float64).sum())


def test_host_layer_fast_math(hiplib):
    """fast_math = true through load_dict sets BF_FLAG_FAST: the integrator's statistics show the fast build, and the film obeys
    the contract against the same scene rendered exact"""
    import beifong_amd.mitsuba as mi
    mi.set_variant("scalar_rgb")
    from beifong_amd.mitsuba.core import Transform4f as T
    from beifong_amd.mitsuba.core.xml import load_dict
    bsdf = {"type": "twosided", "bsdf": {"type": "diffuse", "reflectance": {"type": "spectrum", "value": 1}}}
    films = {}
    for fast in (False, True):
        sen = load_dict({"type": "perspective", "near_clip": 0.2, "far_clip": 10.2, "fov_axis": "x", "fov": 45,
                         "sampler": {"type": "independent", "sample_count": 1 << 15},
                         "film": {"type": "hdrfilm", "width": 1, "height": 1, "rfilter": {"type": "box"}},
                         "to_world": T.look_at([0, 0, 0], [0, -1, 0], [0, 0, 1])})
        scene = load_dict({"type": "scene",
                           "integrator": {"type": "range", "dr": 0.2, "bins": 50, "fast_math": fast, "integrator": {"type": "pathlength"}},
                           "sensor": sen,
                           "emitter": {"type": "rectangle", "to_world": T.look_at([0, 0, 0], [0, -1, 0], [0, 0, 1]) * T.scale([0.02, 0.05, 1]),
                                       "emitter": {"type": "area", "radiance": {"type": "spectrum", "value": 100}}},
                           "target": {"type": "rectangle", "to_world": T.look_at([0, -4, 0], [0, 0, 0], [0, 0, 1]), "bsdf": bsdf},
                           "gnd": {"type": "rectangle", "to_world": T.translate([0, 0, -1]) * T.scale([10, 10, 1]), "bsdf": bsdf}})
        sen = scene.sensors()[0]
        integ = scene.integrator()
        lp = integ.launch_for(sen)
        assert bool(lp.flags & FAST) == fast
        integ.render(scene, sen)
        st, _ = integ.stats()
        assert bool(st.kernel_variant & capi.BF_VARIANT_FAST) == fast
        films[fast] = np.array(sen.film().bitmap(raw=True), np.float64).reshape(-1)
        if fast:
            _host_contract("host fast_math", scene.flat_desc(sen), lp, films[True])
    assert films[True][4] == films[False][4] == 1 << 15


def test_bfrender_fast(hiplib, tmp_path):
    """bfrender --fast writes a histogram that obeys the contract's whole-histogram bound"""
    import beifong_amd.mitsuba as mi
    mi.set_variant("scalar_rgb")
    from beifong_amd.mitsuba.core.xml import load_string
    from tests.test_host import HOST, TRANS_RAD_LIKE
    p = tmp_path / "scene.xml"
    p.write_text(TRANS_RAD_LIKE)
    out = {}
    for fast in (False, True):
        o = tmp_path / f"out{int(fast)}.npy"
        r = subprocess.run([os.path.join(HOST, "bfrender"), "-m", "scalar_rgb", "-Dspp=20000", "-o", str(o)] + (["--fast"] if fast else [])
                           + [str(p)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        out[fast] = np.load(o).reshape(-1)
    scene = load_string(TRANS_RAD_LIKE, spp=20000)
    sen = scene.sensors()[0]
    lp = scene.integrator().launch_for(sen)
    assert not lp.flags & FAST
    _host_contract("bfrender --fast", scene.flat_desc(sen), lp, out[True])
    assert np.any(out[True] != out[False])
