"""Returns by target class (BF_FLAG_CLASSES): a render writes one histogram per class of the scene's class table,
the class of a path being that of the shape its first ray hit.  Expected cells come from the unchanged oracle through
tests/class_ref.py: the class of every path from its composed first hit, the class blocks from every path rendered alone.
Every block of every device histogram is held to its per-cell fp32 summation bound; unpopulated cells are exactly zero and the
count channels exact per class."""
import ctypes as C
import functools

import numpy as np
import pytest

from beifong_amd import capi, motion, scenes
from tests import class_ref as cr
from tests.hist_bound import assert_two_fp32_sums
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _same_records
from tests.scene_builders import oracle_rfilter

pytestmark = pytest.mark.gpu

N, BINS, SPAN = 4096, 64, 25.6
RAGGED = N + 37
CLS = capi.BF_FLAG_CLASSES
# C4: TX aperture, ground, bus, car, motorbike; one class per shape and one for the paths that leave the scene
SIX = ([0, 1, 2, 3, 4], 6, 5)


def _c4_launch(n_paths=N, bins=BINS, mode=capi.BF_MODE_RANGE, color=capi.BF_COLOR_RGB, seed=3, flags=0):
    return capi.make_launch(mode, n_paths, seed=seed, bins=0 if mode == capi.BF_MODE_PATH else bins, bin_width=SPAN / bins, color_mode=color,
                            flags=flags)


@functools.lru_cache(maxsize=None)
def _c4():
    return scenes.multi_mesh_radar(n_paths=N, bins=BINS, dr=SPAN / BINS, seed=3, scale=0.01)[0]


@functools.lru_cache(maxsize=None)
def _c4_singles(bins, mode, color):
    """the RAGGED single-path histograms of a C4 launch: every shorter launch of the same seed is a prefix"""
    return cr.single_path_hists(_c4(), _c4_launch(RAGGED, bins, mode, color))


@functools.lru_cache(maxsize=None)
def _c4_expected(n_paths=N, bins=BINS, mode=capi.BF_MODE_RANGE, color=capi.BF_COLOR_RGB):
    return cr.expected(_c4(), _c4_launch(n_paths, bins, mode, color), *SIX, singles=_c4_singles(bins, mode, color))


def _class_sums_equal_plain(h, h0, exp, lp, add, what):
    """the blocks add up to the plain histogram: the float64 sum of the fp32 blocks lies within sum_k gamma_{N_k - 1} S_k <=
    gamma_{N - 1} S of the exact sum, the plain histogram too; the count channels (A and W; none under a wide filter) exactly"""
    total = capi.split_classes(h, lp, exp.n_classes).astype(np.float64).sum(0)
    assert_two_fp32_sums(total, h0, add.S, add.N, what, counts=exp.counts)


@pytest.mark.parametrize("color", [capi.BF_COLOR_RGB, capi.BF_COLOR_MONO], ids=["rgb", "mono"])
def test_c4_range_mode(hiplib, color):
    sd = _c4()
    lp = _c4_launch(color=color)
    exp, rec_o, add = _c4_expected(color=color)
    pop = exp.population()
    assert pop[0] == 0 and min(pop[1:5]) >= 100 and pop.sum() == N, pop      # ground, bus, car, motorbike: nothing is vacuous
    g = capi.Scene(sd)
    h0, r0, s0 = g.render(lp, records=True)
    g.set_classes(*SIX)
    assert g.channels(lp) == 5 + BINS and g.channels(cr.classed(lp)) == 6 * (5 + BINS)
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and not st.kernel_variant & capi.BF_VARIANT_LEAN and st.n_invalid == 0
    exp.check(h, f"C4 six classes, colour {color}")
    blocks = capi.split_classes(h, lp, 6)
    assert np.array_equal(blocks[:, 4], pop) and np.count_nonzero(blocks[2:5, 5:]) >= 6
    _class_sums_equal_plain(h, h0, exp, lp, add, "C4 six classes against the plain render")
    # the plain render on the same handle, before and after: the same paths, no class bit
    h1, r1, s1 = g.render(lp, records=True)
    _same_records(r0, rec_o)
    _same_records(r1, rec_o)
    assert not (s0.kernel_variant | s1.kernel_variant) & capi.BF_VARIANT_CLASS
    assert_two_fp32_sums(h0, h1, add.S, add.N, "plain render before and after", counts=cr.count_channels(lp))
    # a second table: the three meshes in one class
    g.set_classes([0, 1, 2, 2, 2], 4, 3)
    hm, _, _ = g.render(cr.classed(lp))
    exp.merged([0, 1, 2, 2, 2, 3]).check(hm, "C4, meshes merged")
    # everything in one class of one: the plain render
    g.set_classes([0] * 5, 1, 0)
    ha, ra, _ = g.render(cr.classed(lp), records=True)
    _same_records(ra, rec_o)
    assert ha.size == h0.size
    assert_two_fp32_sums(ha, h0, add.S, add.N, "one class of one against the plain render", counts=cr.count_channels(lp))


ROUTES = ["default", "no_tail", "small_pool", "megakernel", "global_atomics"]


def test_routes_of_one_launch(hiplib, monkeypatch):
    """The same ragged launch (4096 + 37 paths) through every route a class can travel: the tail's load of the slot state, wf_shade /
    wf_trace to the end, slots that regenerate (the class must reset), the one-kernel variant, global atomics.  Every route against
    the expected cells, and the routes pairwise."""
    exp, rec_o, _ = _c4_expected(RAGGED)
    hists = {}
    for route in ROUTES:
        with monkeypatch.context() as m:
            if route == "no_tail":
                m.setenv("BF_WF_TAIL", "0")
            if route == "small_pool":
                m.setenv("BF_WF_POOL", "1024")
            g = capi.Scene(_c4())            # (after setenv: the tunables are read when the scene is created)
        lp = _c4_launch(RAGGED, flags=CLS | {"megakernel": capi.BF_FLAG_MEGAKERNEL, "global_atomics": capi.BF_FLAG_GLOBAL_ATOMICS}.get(route, 0))
        g.set_classes(*SIX)
        h, rec, st = g.render(lp, records=True)
        _same_records(rec, rec_o)
        assert st.kernel_variant & capi.BF_VARIANT_CLASS and st.n_paths == RAGGED, route
        if route == "no_tail":
            assert st.n_bounces_tail == 0 and st.n_bounce_iters > 1
        if route == "default":
            assert st.n_bounces_tail > 0
        exp.check(h, f"route {route}")
        for other, ho in hists.items():
            exp.check_two(h, ho, f"route {route} against {other}")
        hists[route] = h
        g.close()
    assert len(hists) == len(ROUTES)


def test_global_atomics_by_size(hiplib):
    """2560 bins: 2565 floats fit the LDS, six classes of them (15390 > kMaxLdsHist = 12288) do not"""
    bins = 2560
    lp = _c4_launch(N, bins)
    exp, rec_o, add = cr.expected(_c4(), lp, *SIX)
    g = capi.Scene(_c4())
    g.set_classes(*SIX)
    assert g.channels(lp) == 2565 and g.channels(cr.classed(lp)) == 15390
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    exp.check(h, "2560 bins x 6 classes")
    h0, _, _ = g.render(lp)
    _class_sums_equal_plain(h, h0, exp, lp, add, "2560 bins x 6 classes against the plain render (LDS)")
    # two classes fit again: the LDS route of the same launch
    g.set_classes([0, 0, 1, 1, 1], 2, 0)
    assert g.channels(cr.classed(lp)) == 5130
    h2, _, _ = g.render(cr.classed(lp))
    exp.merged([0, 0, 1, 1, 1, 0]).check(h2, "2560 bins x 2 classes")


def test_time_mode_through_the_flux_meter(hiplib):
    sd, lp = scenes.trans_rad(spp=N)
    table = ([0, 1, 2], 4, 3)            # aperture, target, ground, miss
    exp, rec_o, add = cr.expected(sd, lp, *table)
    pop = exp.population()
    assert pop[0] == 0 and min(pop[1:]) >= 100, pop
    g = capi.Scene(sd)
    g.set_classes(*table)
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS
    exp.check(h, "time mode, flux meter")
    _class_sums_equal_plain(h, g.render(lp)[0], exp, lp, add, "time mode against the plain render")
    hm, _, _ = g.render(cr.classed(lp, capi.BF_FLAG_MEGAKERNEL))
    exp.check(hm, "time mode, one-kernel variant")


def test_path_mode(hiplib):
    lp = _c4_launch(mode=capi.BF_MODE_PATH)
    exp, rec_o, add = _c4_expected(mode=capi.BF_MODE_PATH)
    g = capi.Scene(_c4())
    g.set_classes(*SIX)
    h, rec, _ = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert h.size == 30
    exp.check(h, "path mode")
    _class_sums_equal_plain(h, g.render(lp)[0], exp, lp, add, "path mode against the plain render")


@pytest.mark.parametrize("wide", [False, True], ids=["box", "gaussian"])
def test_film(hiplib, wide):
    sd, lp = cr.film_scene()
    if wide:
        sd.sensor.rfilter = oracle_rfilter("gaussian", 0.6, block_size=4)
        sd.finalize()
    table = ([0, 1, 2], 4, 3)            # TX aperture, ground, bus, miss
    exp, rec_o, add = cr.expected(sd, lp, *table)
    assert min(exp.population()[1:]) >= 100
    if wide:
        assert len(exp.counts) == 0      # the count channels' addends are weights
    g = capi.Scene(sd)
    g.set_classes(*table)
    assert g.channels(cr.classed(lp)) == 4 * 48 * (5 + 64)
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and bool(st.kernel_variant & capi.BF_VARIANT_WIDE) == wide
    exp.check(h, f"8 x 6 film, wide {wide}")
    hg, _, _ = g.render(cr.classed(lp, capi.BF_FLAG_GLOBAL_ATOMICS))
    exp.check(hg, f"8 x 6 film, wide {wide}, global atomics")
    exp.check_two(h, hg, f"8 x 6 film, wide {wide}: default against global atomics")
    _class_sums_equal_plain(h, g.render(lp)[0], exp, lp, add, f"film, wide {wide}, against the plain render")


@pytest.mark.parametrize("case", ["raw_phase_bins", "iq_adc_window"])
def test_receive_modes(hiplib, case):
    def build():
        sd, lp = cr.receive_scene()
        if case == "iq_adc_window":
            sd.sensor.window_offset_t, sd.sensor.window_t_bins, sd.sensor.window_offset_f, sd.sensor.window_f_bins = 5, 40, 0, 1
            sd.finalize()
        return sd, lp
    sd, lp = build()
    if case == "iq_adc_window":
        lp.mode, lp.bins = capi.BF_MODE_RECEIVE_IQ, 40
    else:
        lp.phase_bins = 4
    table = ([0, 0, 1, 2], 4, 3)         # both apertures, ground, bus, miss
    exp, rec_o, add = cr.expected(sd, lp, *table, twin=cr.fluxmeter_twin(build))
    pop = exp.population()
    assert pop[0] == 0 and min(pop[1:]) >= 100, pop
    g = capi.Scene(sd)
    g.set_classes(*table)
    cell = 3 + lp.phase_bins
    assert g.channels(cr.classed(lp)) == 4 * lp.bins * cell
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and st.n_invalid == OracleScene(sd).render(lp)[2].n_invalid
    exp.check(h, case)
    # the bus returns something, and in the cells the oracle says
    live = exp.N[2].reshape(-1, cell)[:, 0] > 0
    assert live.any() and np.array_equal(capi.split_classes(h, lp, 4)[2].reshape(-1, cell)[:, 0] != 0, live)
    _class_sums_equal_plain(h, g.render(lp)[0], exp, lp, add, f"{case} against the plain render")
    hm, _, _ = g.render(cr.classed(lp, capi.BF_FLAG_MEGAKERNEL))
    exp.check(hm, f"{case}, one-kernel variant")


def _mesh_vertices(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()


def test_batch_with_seeds_and_mesh_offsets(hiplib):
    sd = _c4()
    lp = _c4_launch()
    seeds = [3, 31, 32]
    offsets = np.array([[0.0, 0.0, 0.0], [0.5, -0.25, 0.0], [-1.0, 0.5, 0.125]], np.float32)
    g = capi.Scene(sd)
    g.set_classes(*SIX)
    hb, rb, st = g.render_batch(cr.classed(lp), 3, seeds=seeds, offsets=offsets, records=True)
    exps = []
    assert hb.shape == (3, 6 * (5 + BINS)) and st.kernel_variant & capi.BF_VARIANT_CLASS
    for k in range(3):
        # the description render k sees: every mesh at fl(p + offset)
        want = motion.deformed_description(sd, {m: (_mesh_vertices(sd, m) + offsets[k][None, :]).astype(np.float32) for m in (2, 3, 4)})
        lk = copy_launch(lp, seed=seeds[k])
        exp, rec_o, _ = _c4_expected() if k == 0 else cr.expected(want, lk, *SIX)
        _same_records(rb[k], rec_o)
        exp.check(hb[k], f"batch render {k}")
        exps.append(exp)
    # the same batch without an LDS histogram: the base channels of render k, class c go through entry [k][c] of the workgroup's class table
    hg, rg, _ = g.render_batch(cr.classed(lp, capi.BF_FLAG_GLOBAL_ATOMICS), 3, seeds=seeds, offsets=offsets, records=True)
    for k in range(3):
        _same_records(rg[k], rb[k])
        exps[k].check(hg[k], f"batch render {k}, global atomics")
        exps[k].check_two(hg[k], hb[k], f"batch render {k}: global atomics against LDS")


def _bike_poses(sd):
    """three poses: as described, and the motorbike (shape 4) driven twice further across the front of the car (shape 3)"""
    xf = np.tile(motion.rigid(), (3, len(sd.shapes), 1, 1)).astype(np.float32)
    xf[1, 4] = motion.rigid(t=(0.5, -1.75, 0.0))
    xf[2, 4] = motion.rigid(t=(1.0, -3.5, 0.0))
    return xf


def test_motion_batch(hiplib):
    sd = _c4()
    lp = _c4_launch()
    xf = _bike_poses(sd)
    g = capi.Scene(sd)
    g.set_classes(*SIX)
    hb, rb, st = g.render_motion_batch(cr.classed(lp), xf, records=True)
    assert hb.shape == (3, 6 * (5 + BINS)) and st.kernel_variant & capi.BF_VARIANT_CLASS
    pops, exps = [], []
    for k in range(3):
        exp, rec_o, _ = _c4_expected() if k == 0 else cr.expected(motion.moved_description(sd, xf[k]), lp, *SIX)
        _same_records(rb[k], rec_o)
        exp.check(hb[k], f"motion batch render {k}")
        pops.append(exp.population())
        exps.append(exp)
    hg, _, _ = g.render_motion_batch(cr.classed(lp, capi.BF_FLAG_GLOBAL_ATOMICS), xf)
    for k in range(3):
        exps[k].check(hg[k], f"motion batch render {k}, global atomics")
    # the motorbike moves in front of the car: the car loses first hits, pose by pose
    assert pops[0][3] != pops[1][3] and pops[1][3] != pops[2][3] and not np.array_equal(pops[0], pops[2]), pops
    # the handle's own geometry and table are as they were
    exp0, rec0, _ = _c4_expected()
    h, rec, _ = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec0)
    exp0.check(h, "after the motion batch")


def test_deform_batch(hiplib):
    sd = _c4()
    lp = _c4_launch()
    v = _mesh_vertices(sd, 4)
    c = 0.5 * (v.min(0) + v.max(0))
    pos = np.stack([v, ((v - c) * np.array([1.0, 1.0, 1.5], np.float32) + c + np.array([0.0, -1.0, 0.0], np.float32))]).astype(np.float32)
    g = capi.Scene(sd)
    g.set_classes(*SIX)
    hb, rb, st = g.render_deform_batch(cr.classed(lp), {4: pos}, records=True)
    assert hb.shape == (2, 6 * (5 + BINS)) and st.kernel_variant & capi.BF_VARIANT_CLASS
    for k in range(2):
        exp, rec_o, _ = _c4_expected() if k == 0 else cr.expected(motion.deformed_description(sd, {4: pos[k]}), lp, *SIX)
        _same_records(rb[k], rec_o)
        exp.check(hb[k], f"deform batch frame {k}")


def test_life_of_the_table(hiplib):
    import torch
    sd = _c4()
    lp = _c4_launch()
    exp, rec_o, add = _c4_expected()
    g = capi.Scene(sd)
    g.set_classes(*SIX)
    # two renders on one stream with a new table between them: it takes effect for the second only
    stream = torch.cuda.Stream()
    buf = torch.zeros((2, 6 * (5 + BINS)), dtype=torch.float32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g.render_device(cr.classed(lp), buf[0].data_ptr(), stream=stream.cuda_stream)
    g.set_classes([0, 1, 2, 2, 2], 4, 3, stream=stream.cuda_stream)
    g.render_device(cr.classed(lp), buf[1].data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    both = buf.cpu().numpy()
    exp.check(both[0], "before the new table")
    merged = exp.merged([0, 1, 2, 2, 2, 3])
    merged.check(both[1][:4 * (5 + BINS)], "after the new table")
    assert not both[1][4 * (5 + BINS):].any()
    # a clone carries the table
    c = g.clone()
    assert c.channels(cr.classed(lp)) == 4 * (5 + BINS)
    merged.check(c.render(cr.classed(lp))[0], "clone")
    c.set_classes(*SIX)                  # ... its own copy
    assert g.channels(cr.classed(lp)) == 4 * (5 + BINS)
    merged.check(g.render(cr.classed(lp))[0], "the original after its clone changed tables")
    c.close()
    # endpoint updates, mesh transforms and rebuilds leave it alone
    g.update_endpoints(sd)
    merged.check(g.render(cr.classed(lp))[0], "after update_endpoints")
    ident = np.tile(motion.rigid(), (len(sd.shapes), 1, 1)).astype(np.float32)
    g.transform_meshes(ident)
    g.rebuild_bvh()
    h, rec, _ = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    merged.check(h, "after transform_meshes and rebuild_bvh")
    # clearing it restores the plain count, and the flag has nothing to split by
    g.clear_classes()
    assert g.channels(cr.classed(lp)) == g.channels(lp) == 5 + BINS
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_CLASSES"):
        g.render(cr.classed(lp))
    assert_two_fp32_sums(g.render(lp)[0], OracleScene(sd).render(lp)[0], add.S, add.N, "plain render after clear_classes")


def _status(lib, fn, *args):
    st = fn(*args)
    return st, (lib.bf_last_error() or b"").decode()


def test_refusals(hiplib):
    import torch
    lib = hiplib
    sd = _c4()
    lp = _c4_launch()
    g = capi.Scene(sd)
    INVALID, UNSUPPORTED = 1, capi.BF_ERR_UNSUPPORTED
    assert capi.BF_ERR_INVALID == INVALID
    # bf_scene_set_classes
    for args in ((2, [0, 1, 2, 0, 0], 0), (2, [0, 1, 1, 0, 0], 2), (capi.BF_MAX_CLASSES + 1, [0] * 5, 0)):
        a = np.asarray(args[1], np.uint32)
        st, msg = _status(lib, lib.bf_scene_set_classes, g.handle, args[0], a.ctypes.data_as(C.c_void_p), args[2], None)
        assert st == INVALID and "bf_scene_set_classes" in msg, (args, st, msg)
    g.set_classes([0] * 5, capi.BF_MAX_CLASSES, capi.BF_MAX_CLASSES - 1)
    g.clear_classes()
    # the flag without a table
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_CLASSES.*no class table"):
        g.render(cr.classed(lp))
    g.set_classes(*SIX)
    for extra, name in ((capi.BF_FLAG_FAST, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, "BF_FLAG_MOMENT")):
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_CLASSES.*{name}"):
            g.render(cr.classed(lp, extra))
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        capi.render_sharded([g], cr.classed(lp))
    buf = torch.zeros(6 * (5 + BINS), dtype=torch.float32, device="cuda")
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        capi.render_sharded_device([g], cr.classed(lp), [buf.data_ptr()])
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        g.render_converge(cr.classed(lp), 0.1, max_rounds=2)
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        g.render_converge_device(cr.classed(lp), buf.data_ptr(), 0.1, max_rounds=2)
    # the motion / deform batch entries refuse before they prepare anything
    xf = _bike_poses(sd)
    pos = np.stack([_mesh_vertices(sd, 4)] * 2)
    for extra, status, name in ((capi.BF_FLAG_FAST, INVALID, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, INVALID, "BF_FLAG_MOMENT")):
        with pytest.raises(capi.BeifongError, match=rf"status {status}\).*BF_FLAG_CLASSES.*{name}"):
            g.render_motion_batch(cr.classed(lp, extra), xf)
        with pytest.raises(capi.BeifongError, match=rf"status {status}\).*BF_FLAG_CLASSES.*{name}"):
            g.render_deform_batch(cr.classed(lp, extra), {4: pos})
    g.clear_classes()
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_CLASSES.*no class table"):
        g.render_motion_batch(cr.classed(lp), xf)
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_CLASSES.*no class table"):
        g.render_deform_batch(cr.classed(lp), {4: pos})
    g.set_classes(*SIX)
    # a rolling render: refused, and the open sequence stays intact
    seq = _Sequence(g, lp, [5, 6])
    seq.issue([0])
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES.*BF_FLAG_ROLLING"):
        g.render_device(cr.classed(lp, capi.BF_FLAG_ROLLING), buf.data_ptr())
    seq.issue([1])
    g.flush()
    h, recs = seq.results()
    assert float(buf.abs().sum()) == 0.0
    osc = OracleScene(sd)
    for k, seed in enumerate([5, 6]):
        _, ro, _, add = osc.render(copy_launch(lp, seed=seed), records=True, threads=8, addends=True)
        _same_records(recs[k], ro)
        from tests.hist_bound import assert_fp32_sum
        assert_fp32_sum(h[k], add.ref, add.S, add.N, f"rolling render {k} around the refusal", counts=cr.count_channels(lp))
    # the table survived all of it
    exp, _, _ = _c4_expected()
    exp.check(g.render(cr.classed(lp))[0], "after the refusals")


def test_motion_sweep_with_classes(hiplib):
    """Two targets at two speeds over 8 pulses: the cube gains a class axis behind the pulse axis, and its classes add up to the
    unclassed cube within twice the summation bound (two fp32 summations of the same addends)."""
    pytest.importorskip("torch")
    from beifong_amd import sweep
    from tests.test_gpu_motion import _identity, _two_plates
    n_pulses = 8
    sd, lp, plates = _two_plates(-0.004, -0.0125)
    lp = copy_launch(lp, n_paths=1 << 12)
    xf = np.tile(_identity(sd)[None], (n_pulses, 1, 1, 1))
    for i, (k, dx) in enumerate(zip(plates, (-0.004, -0.0125))):
        xf[:, k, 0, 3] = dx * np.arange(n_pulses)
    shape_class = np.zeros(len(sd.shapes), np.uint32)
    shape_class[plates[0]], shape_class[plates[1]] = 1, 2
    cube = sweep.render_motion_sweep(sd, lp, xf, n_streams=2, classes=(shape_class, 4, 3))
    plain = sweep.render_motion_sweep(sd, lp, xf, n_streams=2)
    cells = lp.bins * lp.bins_y
    assert cube.shape == (n_pulses, 4, cells, 3) and plain.shape == (n_pulses, cells, 3)
    assert sweep.range_doppler(cube[:, 1]).shape == (n_pulses, cells)
    assert np.array_equal(cube[..., 2].sum(1), plain[..., 2])                   # W: exact
    assert min(cube[0, 1, :, 2].sum(), cube[0, 2, :, 2].sum()) > 0              # both plates are first hits of some paths
    for k in range(n_pulses):
        add = OracleScene(motion.moved_description(sd, xf[k])).render(lp, threads=8, addends=True)[3]
        assert_two_fp32_sums(cube[k].astype(np.float64).sum(0), plain[k], add.S, add.N, f"pulse {k}: classes summed against the unclassed cube")
