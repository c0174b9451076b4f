"""BF_FLAG_MOMENT on the GPU: next to every first-moment channel the sum of the squared samples (moment.cpp).

Expected second moments come from the oracle as it is, without the flag (tests/moment_ref.py): from the per-path records
of one oracle render where the sensor weight is 1 and the film 1 x 1, from the oracle rendering every path alone
otherwise.  Every m2_ cell is held to gamma_N E + 2 N 2^-126 (gamma_{N+8} / gamma_{N+4} where the helper says so), every
first-moment cell to the bound of tests/hist_bound.py, two device results of one launch to twice that."""
import functools
import os
import subprocess

import numpy as np
import pytest

from beifong_amd import capi, scenes
from tests import moment_ref as mr
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _launch_like, _same_records, _Sequence
from tests.scene_builders import oracle_rfilter
from tests.test_host import HOST

pytestmark = pytest.mark.gpu
M = capi.BF_FLAG_MOMENT
BINS, DR = 64, 0.4


@functools.lru_cache(maxsize=None)
def _bus():
    sd, _ = scenes.bus_radar(n_tris=20000, n_paths=4096, bins=BINS, dr=DR)
    return sd, capi.Scene(sd), OracleScene(sd)


def _bus_launch(mode=capi.BF_MODE_RANGE, color=capi.BF_COLOR_RGB, n_paths=4096, seed=1, flags=M, path_offset=0):
    w = {capi.BF_MODE_RANGE: DR, capi.BF_MODE_TIME: DR / 3.0e8, capi.BF_MODE_PATH: 0.0}[mode]
    return capi.make_launch(mode, n_paths, seed=seed, path_offset=path_offset, bins=0 if mode == capi.BF_MODE_PATH else BINS, bin_width=w,
                            color_mode=color, flags=flags)


@functools.lru_cache(maxsize=None)
def _bus_expected(mode, color, n_paths=4096, seed=1, path_offset=0):
    """(oracle records, Expected) of one bus launch: first moments from the oracle's Addends, second from its records"""
    _, _, osc = _bus()
    lp = _bus_launch(mode, color, n_paths, seed, flags=0, path_offset=path_offset)
    _, rec, _, add = osc.render(lp, records=True, threads=8, addends=True)
    return rec, mr.Expected(lp, add.ref, add.S, add.N, mr.from_records(rec, lp), weight_one=True)


@pytest.mark.parametrize("color", [capi.BF_COLOR_RGB, capi.BF_COLOR_MONO], ids=["rgb", "mono"])
@pytest.mark.parametrize("mode", [capi.BF_MODE_RANGE, capi.BF_MODE_TIME, capi.BF_MODE_PATH], ids=["range", "time", "path"])
def test_modes_against_the_oracle(hiplib, mode, color):
    _, g, _ = _bus()
    lp = _bus_launch(mode, color)
    rec_o, exp = _bus_expected(mode, color)
    h, rec, st = g.render(lp, records=True)
    _same_records(rec, rec_o)
    assert h.size == 5 + 2 * (mr.n_aov(lp) + 3) and h[4] == 4096 and st.n_invalid == 0
    assert st.kernel_variant & capi.BF_VARIANT_MOMENT
    exp.check(h, f"moment mode {mode} colour {color}")
    _, second = capi.moment_layout(lp)
    assert np.count_nonzero(h[second]) >= (3 if mode == capi.BF_MODE_PATH else 8)
    # the flag changes nothing else: the render without it, and its variant word
    h0, rec0, st0 = g.render(mr.plain(lp), records=True)
    _same_records(rec0, rec_o)
    assert not st0.kernel_variant & capi.BF_VARIANT_MOMENT
    assert np.array_equal(h0[3:5], h[3:5])


def test_fluxmeter_squares_are_of_the_unweighted_values(hiplib):
    """C1 (fluxmeter: ray weight pi, time mode): the time bins hold the UNWEIGHTED XYZ, and so do their squares"""
    sd, lp = scenes.trans_rad(spp=2048)
    osc = OracleScene(sd)
    ref, S, N, E2 = mr.single_paths(osc, lp)
    exp = mr.Expected(lp, ref, S, N, mr.m2_from_single(E2, N, lp), weight_one=False)
    h, rec, _ = capi.Scene(sd).render(mr.with_moment(lp), records=True)
    _same_records(rec, osc.render(lp, records=True)[1])
    exp.check(h, "fluxmeter time bins")
    first, second = capi.moment_layout(mr.with_moment(lp))
    live = np.flatnonzero(h[first[0, :150]])
    assert live.size >= 6
    # nested.Y is the unweighted Y: the base Y carries the factor pi
    assert np.isclose(h[1], np.pi * h[first[0, 151]], rtol=1e-5) and h[second[0, 151]] > 0


def _film(bins, wide=False):
    sd, lp = scenes.film_half_lit(film=(8, 6), spp=64, mode=capi.BF_MODE_RANGE, bins=bins, dr=6.4 / bins)
    if wide:
        sd.sensor.rfilter = oracle_rfilter("gaussian", 0.6, block_size=4)
        sd.finalize()
    return sd, lp


@functools.lru_cache(maxsize=None)
def _film_expected(bins, wide=False):
    sd, lp = _film(bins, wide)
    ref, S, N, E2 = mr.single_paths(OracleScene(sd), lp, wide=wide)
    # wide filter: no exact count channels (their addends are weights), m2 addends recovered as (w x)^2 / w: gamma_{N+4}
    return mr.Expected(lp, ref, S, N, mr.m2_from_single(E2, N, lp, extra=4 if wide else 0, weight_one=True), weight_one=True,
                       counts=[] if wide else None)


def test_film_across_the_lds_boundary(hiplib):
    """8 x 6 film, 128 range bins: 6384 floats without the flag (LDS), 48 (5 + 2 * 131) = 12816 > kMaxLdsHist with it"""
    sd, lp = _film(128)
    g = capi.Scene(sd)
    lm = mr.with_moment(lp)
    assert g.channels(lp) == 6384 and g.channels(lm) == 12816
    exp = _film_expected(128)
    h, _, st = g.render(lm)
    exp.check(h, "film 128 bins (global atomics by size)")
    # the oracle's own count: one of the 3072 position samples rounds out of the film's first row and is dropped there too
    ho, _, so = OracleScene(sd).render(lp)
    assert st.n_invalid == so.n_invalid and np.array_equal(h.reshape(48, -1)[:, 4], ho.reshape(48, -1)[:, 4])
    assert h.reshape(48, -1)[:, 4].sum() + st.n_invalid == 3072
    h0, _, _ = g.render(lp)
    exp.check_two(np.where(_second_mask(lm), 0.0, h), _widen(h0, lp), "film 128 bins: first moments, flag against no flag")
    # 32 bins fit the LDS with the flag: both routes of the same launch
    sd, lp = _film(32)
    g = capi.Scene(sd)
    exp = _film_expected(32)
    h_lds, _, _ = g.render(mr.with_moment(lp))
    h_glb, _, _ = g.render(mr.with_moment(lp, capi.BF_FLAG_GLOBAL_ATOMICS))
    exp.check(h_lds, "film 32 bins LDS")
    exp.check(h_glb, "film 32 bins global atomics")
    exp.check_two(h_lds, h_glb, "film 32 bins LDS against global atomics")
    _, second = capi.moment_layout(mr.with_moment(lp))
    assert np.count_nonzero(h_lds[second]) > 48


def _second_mask(lm):
    """the channels a render without the flag does not have: m2_ and nested.XYZ"""
    cells, c0, c1 = mr.cells_of(lm)
    m = np.zeros(cells * c1, bool)
    first, second = capi.moment_layout(lm)
    m[second.reshape(-1)] = True
    if c1 - c0 >= 6:
        m[(np.arange(cells)[:, None] * c1 + c0 + np.arange(3)[None, :]).reshape(-1)] = True      # nested.XYZ too
    return m


def _widen(h0, lp):
    """a histogram without the flag laid out in the moment layout (zeros elsewhere)"""
    cells, c0, c1 = mr.cells_of(lp)
    out = np.zeros((cells, c1))
    out[:, :c0] = np.asarray(h0).reshape(cells, c0)
    return out.reshape(-1)


def test_film_with_a_wide_filter(hiplib):
    sd, lp = _film(32, wide=True)
    exp = _film_expected(32, wide=True)
    h, _, st = capi.Scene(sd).render(mr.with_moment(lp))
    assert st.kernel_variant & capi.BF_VARIANT_WIDE and st.kernel_variant & capi.BF_VARIANT_MOMENT
    exp.check(h, "film 32 bins, gaussian filter")
    _, second = capi.moment_layout(mr.with_moment(lp))
    assert np.count_nonzero(h[second]) > 48


def test_rolling_sequences_in_both_base_table_regimes(hiplib):
    """3 renders (all inside the LDS window or just behind it) and 40 renders of 256 paths (beyond kRollBase = 32: the oldest
    renders' late samples take global atomics, the others the eleven-entry base table)"""
    _, g, _ = _bus()
    for n_paths, seeds in ((4096, [5, 6, 7]), (256, list(range(200, 240)))):
        lp = _bus_launch(n_paths=n_paths)
        seq = _Sequence(g, lp, seeds)
        seq.issue()
        g.flush()
        h, recs = seq.results()
        for k, seed in enumerate(seeds):
            rec_o, exp = _bus_expected(capi.BF_MODE_RANGE, capi.BF_COLOR_RGB, n_paths, seed)
            _same_records(recs[k], rec_o)
            exp.check(h[k], f"rolling {len(seeds)} x {n_paths}, render {k}")
            hs, _, _ = g.render(_bus_launch(n_paths=n_paths, seed=seed))
            exp.check_two(h[k], hs, f"rolling {len(seeds)} x {n_paths}, render {k} against stand-alone")


def test_rolling_render_of_the_other_layout_is_refused(hiplib):
    _, g, _ = _bus()
    lp = _bus_launch(n_paths=4096, flags=0)
    seq = _Sequence(g, lp, [5, 6])
    seq.issue([0])
    import torch
    buf = torch.zeros(g.channels(_bus_launch()), dtype=torch.float32, device="cuda")
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_MOMENT"):
        g.render_device(_bus_launch(seed=9, flags=M | capi.BF_FLAG_ROLLING), buf.data_ptr())
    seq.issue([1])
    g.flush()
    h, recs = seq.results()
    assert float(buf.abs().sum()) == 0.0
    for k, seed in enumerate([5, 6]):
        hs, rs, _ = g.render(_launch_like(lp, seed), records=True)
        _same_records(recs[k], rs)
        _, exp = _bus_expected(capi.BF_MODE_RANGE, capi.BF_COLOR_RGB, 4096, seed)
        assert h[k][4] == 4096
        exp.check_two(_widen(h[k], lp), _widen(hs, lp), f"sequence without the flag, render {k}")      # (the first-moment channels)
    # and the other way round
    seq = _Sequence(g, _bus_launch(), [5])
    seq.issue()
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_MOMENT"):
        g.render_device(_bus_launch(seed=9, flags=capi.BF_FLAG_ROLLING), buf.data_ptr())
    g.flush()
    _bus_expected(capi.BF_MODE_RANGE, capi.BF_COLOR_RGB, 4096, 5)[1].check(seq.results()[0][0], "moment sequence after the refusal")


def test_batch_shards_sharded_and_one_kernel_variant(hiplib):
    _, g, _ = _bus()
    lp = _bus_launch()
    rec_o, exp = _bus_expected(capi.BF_MODE_RANGE, capi.BF_COLOR_RGB)
    hs, _, _ = g.render(lp)
    # a batch of four seeds
    seeds = [1, 21, 22, 23]
    hb, rb, _ = g.render_batch(lp, 4, seeds=seeds, records=True)
    for k, seed in enumerate(seeds):
        rk, ek = _bus_expected(capi.BF_MODE_RANGE, capi.BF_COLOR_RGB, 4096, seed)
        _same_records(rb[k], rk)
        ek.check(hb[k], f"batch render {k}")
    exp.check_two(hb[0], hs, "batch render 0 against stand-alone")
    # two shards by path_offset, summed in fp32: one summation of the same addends
    parts = [g.render(_bus_launch(n_paths=2048, path_offset=2048 * k))[0] for k in range(2)]
    both = parts[0] + parts[1]
    exp.check(both, "two shards summed")
    exp.check_two(both, hs, "two shards against stand-alone")
    # bf_render_sharded on one device
    hh, st = capi.render_sharded([g], lp)
    exp.check(hh, "bf_render_sharded")
    exp.check_two(hh, hs, "bf_render_sharded against stand-alone")
    assert st.n_paths == 4096
    # the one-kernel variant
    hm, rm, st = g.render(_bus_launch(flags=M | capi.BF_FLAG_MEGAKERNEL), records=True)
    _same_records(rm, rec_o)
    exp.check(hm, "one-kernel variant")
    exp.check_two(hm, hs, "one-kernel variant against stand-alone")
    assert st.kernel_variant & capi.BF_VARIANT_MOMENT


def _receive_scene(kind):
    if kind == "plate":
        sd, lp = scenes.plate_doppler(n_paths=1024, t_bins=8)
    else:
        sd, lp = scenes.bus_receive(n_tris=5000, n_paths=1024, t_bins=8, dr=3.2)
        sd.sensor.f_bandwidth = sd.physics.c / (sd.physics.lambda_min_nm * 1e-9)      # spread the band over the four rows
    sd.sensor.f_bins = 4
    sd.finalize()
    lp.bins_y = 4
    return sd, lp


@pytest.mark.parametrize("form", ["raw", "raw_phase4", "iq"])
@pytest.mark.parametrize("kind", ["plate", "wigner"])
def test_receive_modes(hiplib, kind, form):
    sd, lp = _receive_scene(kind)
    lp.mode = capi.BF_MODE_RECEIVE_IQ if form == "iq" else capi.BF_MODE_RECEIVE_RAW
    lp.phase_bins = 4 if form == "raw_phase4" else 0
    osc = OracleScene(sd)
    ref, S, N, E2 = mr.single_paths(osc, lp)
    exp = mr.Expected(lp, ref, S, N, mr.m2_from_single(E2, N, lp), weight_one=False)
    g = capi.Scene(sd)
    lm = mr.with_moment(lp)
    h, rec, st = g.render(lm, records=True)
    _same_records(rec, osc.render(lp, records=True)[1])
    cells, c0, c1 = mr.cells_of(lp)
    assert (cells, h.size) == (32, 32 * c1) and c1 == {"raw": 4, "raw_phase4": 8, "iq": 5}[form]
    exp.check(h, f"receive {kind} {form}")
    first, second = capi.moment_layout(lm)
    assert np.count_nonzero(h[second[:, 0]]) >= 1 and h.reshape(32, c1)[:, 2].sum() + st.n_invalid == 1024
    h0, _, _ = g.render(lp)
    exp.check_two(np.where(_second_mask(lm), 0.0, h), _widen(h0, lp), f"receive {kind} {form}: flag against no flag")
    mean, var, rel = capi.moment_estimate(h, lm)
    assert mean.shape == (32, 2 if form == "iq" else 1)


def test_a_square_that_overflows_drops_the_sample(hiplib):
    """ImageBlock::put refuses a sample with any non-finite channel: radiance 1e25 is finite, its square is not"""
    sd, lp = scenes.film_half_lit(film=(1, 1), spp=64, radiance=1.0e25)
    lp.film_width = lp.film_height = lp.spp = 0
    g = capi.Scene(sd)
    h0, rec0, st0 = g.render(lp, records=True)
    rec_o = OracleScene(sd).render(lp, records=True)[1]
    _same_records(rec0, rec_o)
    assert h0[4] == 64 and st0.n_invalid == 0
    over = np.abs(rec_o["L"].astype(np.float64)) > np.sqrt(float(np.finfo(np.float32).max))
    assert 8 <= over.sum() <= 56
    h, rec, st = g.render(mr.with_moment(lp), records=True)
    _same_records(rec, rec_o)
    assert st.n_invalid == over.sum() and h[4] == 64 - over.sum()
    assert np.all(np.isfinite(h))
    # what is left are the samples with L = 0 here: every other channel is empty
    assert np.all(rec_o["L"][~over] == 0) and np.all(h[[0, 1, 2, 5, 6, 7, 8, 9, 10]] == 0)
    assert h[3] == np.count_nonzero(rec_o["valid"][~over])


def test_fast_arithmetic_is_refused_and_the_handle_stays_usable(hiplib):
    _, g, _ = _bus()
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_FAST"):
        g.render(_bus_launch(flags=M | capi.BF_FLAG_FAST))
    rec_o, exp = _bus_expected(capi.BF_MODE_RANGE, capi.BF_COLOR_RGB)
    h, rec, st = g.render(_bus_launch(), records=True)
    _same_records(rec, rec_o)
    exp.check(h, "after the refusal")
    assert st.kernel_variant & capi.BF_VARIANT_MOMENT and not st.kernel_variant & capi.BF_VARIANT_FAST


HOST_XML = """
<scene version="2.1.0">
    <integrator type="moment">
        <integrator type="range" name="nested"><integrator type="pathlength"/><float name="dr" value="0.25"/><integer name="bins" value="32"/></integrator>
    </integrator>
    <sensor type="perspective">
        <transform name="to_world"><lookat origin="0, 0, 0" target="0, -1, 0" up="0, 0, 1"/></transform>
        <film type="hdrfilm"><integer name="width" value="1"/><integer name="height" value="1"/><rfilter type="box"/></film>
        <sampler type="independent"><integer name="sample_count" value="$spp"/></sampler>
    </sensor>
    <emitter type="spot"><spectrum value="10" name="intensity"/><float name="cutoff_angle" value="25"/>
        <transform name="to_world"><lookat origin="0, 0, 0" target="0, -1, 0" up="0, 0, 1"/></transform></emitter>
    <shape type="rectangle"><transform name="to_world"><lookat origin="0, -4, 0" target="0, 0, 0" up="0, 0, 1"/></transform>
        <bsdf type="twosided"><bsdf type="diffuse"/></bsdf></shape>
    <shape type="rectangle"><transform name="to_world"><scale x="20" y="20"/><lookat origin="0, 0, -0.5" target="0, 0, 0.5"/></transform>
        <bsdf type="twosided"><bsdf type="diffuse"/></bsdf></shape>
</scene>
"""


def test_moment_integrator_through_the_plugin_surface(hiplib, tmp_path):
    from beifong_amd import mitsuba as m
    from beifong_amd.mitsuba import _host
    from beifong_amd.mitsuba.core.xml import load_string
    m.set_variant("scalar_rgb")
    scene = load_string(HOST_XML, spp=2048)
    sensor, integ = scene.sensors()[0], scene.integrator()
    integ.render(scene, sensor)
    bmp = sensor.film().bitmap(raw=True)
    names = integ.aov_names()
    assert len(names) == 2 * 35 and names[0] == "nested.S0.Y" and names[34] == "nested.Z" and names[-1] == "m2_nested.Z"
    assert bmp.channel_names() == ["X", "Y", "Z", "A", "W"] + names
    img = np.array(bmp)
    assert img.shape == (1, 1, 75) and img[0, 0, 4] == 2048
    lp = integ.launch_for(sensor)
    assert lp.flags & M
    sd = scene.flat_desc(sensor)
    hc, rec, _ = capi.Scene(sd).render(lp, records=True)
    # the bitmap and the C-ABI render of the same launch: two fp32 summations of the same addends, each held to the oracle
    l0 = mr.plain(lp)
    _, rec_o, _, add = OracleScene(sd).render(l0, records=True, threads=8, addends=True)
    _same_records(rec, rec_o)
    exp = mr.Expected(l0, add.ref, add.S, add.N, mr.from_records(rec_o, l0), weight_one=True)
    exp.check(img.reshape(-1), "bitmap of the moment integrator")
    exp.check(hc, "C-ABI render of the integrator's launch")
    exp.check_two(img.reshape(-1), hc, "bitmap against the C-ABI render")
    assert np.count_nonzero(img[0, 0, 40:72]) >= 3
    p = tmp_path / "scene.xml"
    p.write_text(HOST_XML)
    out = tmp_path / "out.npy"
    r = subprocess.run([os.path.join(HOST, "bfrender"), "-m", "scalar_rgb", "-Dspp=2048", "-o", str(out), str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    a = np.load(out)
    assert a.shape == (1, 1, 75) and a[0, 0, 4] == 2048
    r = subprocess.run([os.path.join(HOST, "bfrender"), "-m", "scalar_rgb", "-Dspp=2048", str(p)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    img2, names2 = _host.read_exr(str(tmp_path / "scene.exr"))
    assert img2.shape == (1, 1, 75) and set(names2) == set(["X", "Y", "Z", "A", "W"] + names)


def test_relative_standard_error_brackets_the_spread_over_seeds(hiplib):
    """What the estimate means.  STATISTICAL, with its condition: range mode on the bus, 2^14 paths; the bins with at least 64
    non-zero addends (by the oracle, in the render with seed 1: 16 of the 64 bins); rel_stderr of that ONE moment render
    against the relative spread (sample standard deviation, 16 renders) of the bin's mean over 16 seeds whose path ranges
    are disjoint (seed + path index selects the path's stream, so neighbouring seeds share paths).  The two must agree within
    a factor 2 either way.  The spread of 16 means has a relative error of about 1 / sqrt(30) = 18 %, the variance estimate of
    a bin with N >= 64 hits about the same, so a factor 2 is some four standard deviations; the seeds are fixed and every path
    is bit-equal to the oracle's, and the oracle alone, computing the same quantities from its records, gives ratios
    0.58 .. 1.34 for these seeds (asserted below before the device is asked)."""
    _, g, osc = _bus()
    n = 1 << 14
    seeds = [(65 + k) * 1000003 for k in range(16)]
    # the oracle alone
    l1 = _bus_launch(n_paths=n, seed=1, flags=0)
    _, rec, _, add = osc.render(l1, records=True, threads=8, addends=True)
    pick = np.flatnonzero(add.N[5:5 + BINS] >= 64)
    assert pick.size >= 12
    m2 = mr.from_records(rec, l1)
    mean_o = add.ref[5:5 + BINS] / n
    rel_o = np.sqrt(np.maximum(m2.E[:BINS] / n - mean_o ** 2, 0.0) / (n - 1)) / np.abs(mean_o)
    means_o = np.array([osc.render(_bus_launch(n_paths=n, seed=s, flags=0), threads=8, addends=True)[3].ref[5:5 + BINS] / n for s in seeds])
    spread_o = means_o.std(axis=0, ddof=1) / np.abs(means_o.mean(axis=0))
    ratio_o = spread_o[pick] / rel_o[pick]
    assert 0.5 < ratio_o.min() and ratio_o.max() < 2.0, ratio_o
    # the device: one moment render, sixteen more for the spread
    lm = _bus_launch(n_paths=n, seed=1)
    h, _, _ = g.render(lm)
    mean, var, rel = capi.moment_estimate(h, lm)
    means = np.array([capi.moment_estimate(g.render(_bus_launch(n_paths=n, seed=s))[0], lm)[0][0, :BINS] for s in seeds])
    spread = means.std(axis=0, ddof=1) / np.abs(means.mean(axis=0))
    ratio = spread[pick] / rel[0, :BINS][pick]
    assert 0.5 <= ratio.min() and ratio.max() <= 2.0, ratio
    assert np.allclose(ratio, ratio_o, rtol=1e-3)


@pytest.mark.parametrize("form", ["raw_phase4", "iq"])
def test_receive_with_a_wide_filter_on_the_adc(hiplib, form):
    """A tent filter on the ADC (put_wide's receive branch): the cell is Y A W [phase bins] m2_Y — the phase bins have no
    second moment and must be those of the launch without the flag; m2_Y's addend w x^2 is recovered as (w x)^2 / w"""
    sd, lp = _receive_scene("wigner")
    sd.sensor.rfilter = oracle_rfilter("tent")
    sd.finalize()
    lp.mode = capi.BF_MODE_RECEIVE_IQ if form == "iq" else capi.BF_MODE_RECEIVE_RAW
    lp.phase_bins = 4 if form == "raw_phase4" else 0
    osc = OracleScene(sd)
    ref, S, N, E2 = mr.single_paths(osc, lp, wide=True)
    exp = mr.Expected(lp, ref, S, N, mr.m2_from_single(E2, N, lp, extra=4), weight_one=False, counts=[])
    g = capi.Scene(sd)
    lm = mr.with_moment(lp)
    h, rec, st = g.render(lm, records=True)
    _same_records(rec, osc.render(lp, records=True)[1])
    assert st.kernel_variant & capi.BF_VARIANT_WIDE and st.kernel_variant & capi.BF_VARIANT_MOMENT
    exp.check(h, f"receive, tent filter, {form}")
    h0, _, _ = g.render(lp)
    exp.check_two(np.where(_second_mask(lm), 0.0, h), _widen(h0, lp), f"receive, tent filter, {form}: flag against no flag")
    cells, c0, c1 = mr.cells_of(lp)
    first, second = capi.moment_layout(lm)
    assert np.count_nonzero(h[second[:, 0]]) >= 2
    if form == "raw_phase4":
        assert np.count_nonzero(h.reshape(cells, c1)[:, 3:7]) >= 2


def test_motion_batch(hiplib):
    """Per-render rigid transforms (the kernels' kGeom forms): every render against the oracle on the scene rebuilt from the
    moved vertices"""
    from beifong_amd import motion
    from tests.test_gpu_motion import _multi_mesh
    from tests.test_gpu_motion_batch import _batch_poses
    sd, _ = _multi_mesh(True)
    lp = capi.make_launch(capi.BF_MODE_RANGE, 4096, seed=3, bins=BINS, bin_width=DR, color_mode=capi.BF_COLOR_RGB)
    lm = mr.with_moment(lp)
    xf = _batch_poses(sd, 3)
    seeds = [31, 32, 33]
    hb, rb, st = capi.Scene(sd).render_motion_batch(lm, xf, seeds=seeds, records=True)
    assert st.kernel_variant & capi.BF_VARIANT_MOMENT and st.n_paths == 3 * 4096
    assert not np.array_equal(rb[0]["L"], rb[1]["L"])
    for k in range(3):
        l1 = mr.copy_launch(lp, seed=seeds[k])
        _, ro, _, add = OracleScene(motion.moved_description(sd, xf[k])).render(l1, records=True, threads=8, addends=True)
        _same_records(rb[k], ro)
        exp = mr.Expected(l1, add.ref, add.S, add.N, mr.from_records(ro, l1), weight_one=True)
        exp.check(hb[k], f"motion batch render {k}")
        _, second = capi.moment_layout(lm)
        assert np.count_nonzero(hb[k][second]) >= 8


def test_rolling_sequence_across_endpoint_updates(hiplib):
    """The radar turns between the renders of ONE rolling sequence (the kernels' kMulti forms: per-path endpoint tables):
    every frame against the oracle on the scene built for that frame"""
    import torch
    from tests.test_gpu_updates import _mesh, _radar
    mesh = _mesh()
    frames = [_radar(mesh, n_paths=4096, yaw=y) for y in (0.0, 12.0, 24.0)]
    g = capi.Scene(frames[0][0])
    lm0 = mr.with_moment(frames[0][1])
    hist = torch.zeros((3, g.channels(lm0)), dtype=torch.float32, device="cuda")
    rec = torch.zeros((3, 4096, 4), dtype=torch.int32, device="cuda")
    for k, (sd, lp) in enumerate(frames):
        if k:
            g.update_endpoints(sd)
        g.render_device(_launch_like(lp, 500 + k, flags=M | capi.BF_FLAG_ROLLING | capi.BF_FLAG_COUNT), hist[k].data_ptr(),
                        records_ptr=rec[k].data_ptr())
    st = g.flush(want_stats=True)
    assert st.n_paths == 3 * 4096 and st.n_launches_tail <= 1          # the updates joined one sequence
    torch.cuda.synchronize()
    h = hist.cpu().numpy()
    r = rec.cpu().numpy().view(np.uint32).reshape(3, -1, 4)
    for k, (sd, lp) in enumerate(frames):
        l1 = _launch_like(lp, 500 + k)
        _, ro, _, add = OracleScene(sd).render(l1, records=True, threads=8, addends=True)
        _same_records(np.ascontiguousarray(r[k]).view(capi.PATH_RECORD_DTYPE).reshape(-1), ro)
        exp = mr.Expected(l1, add.ref, add.S, add.N, mr.from_records(ro, l1), weight_one=True)
        exp.check(h[k], f"rolling across endpoint updates, frame {k}")
        assert h[k][4] == 4096
    assert not np.array_equal(r[0], r[1])
