"""Returns by range rate (Scene.set_range_rate_classes with BF_FLAG_CLASSES): the class of a path is the bin of the
range rate of its first intersection along its primary ray.  Expected cells come from the unchanged oracle through
tests/range_rate_ref.py (every path's composed primary ray, the shape and the point it meets first -> capi.range_rate_classes ->
class_ref.per_class: every path rendered alone).  Every block of every device histogram is held to its per-cell fp32 summation
bound; unpopulated cells are exactly zero, the count channels exact per class, and the per-path records bit-equal to the oracle's.
The tables, the twists and their populations on these scenes are in tests/range_rate_ref.py; tests/test_range_rate_host.py asserts the
populations on the oracle."""
import ctypes as C
import functools

import numpy as np
import pytest

from beifong_amd import capi, motion, scenes
from tests import arrival_ref as ar
from tests import class_ref as cr
from tests import range_rate_ref as rr
from tests.hist_bound import assert_fp32_sum, assert_two_fp32_sums
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _same_records
from tests.scene_builders import oracle_rfilter

POPULATIONS, SENSOR_LIN, table, twists = rr.POPULATIONS, rr.SENSOR_LIN, rr.table, rr.twists

pytestmark = pytest.mark.gpu

N, NB = 4096, 1024           # paths of a single render; of every render of a batch
RAW, IQ = capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ
CLS = capi.BF_FLAG_CLASSES
SHAPES = ([0, 0, 1, 2], 4, 3)      # the receive scene by shape: both apertures, ground, bus, miss
ARRIVAL = (8, 4, (0.0, 0.6, -0.2, 0.4))


@functools.lru_cache(maxsize=None)
def _rx():
    return cr.receive_scene(N)[0]


@functools.lru_cache(maxsize=None)
def _twin():
    return cr.fluxmeter_twin(cr.receive_scene)


@functools.lru_cache(maxsize=None)
def _tw():
    return twists(_rx())


def _rx_launch(n_paths=N, mode=RAW, seed=5, flags=0):
    return copy_launch(cr.receive_scene(N)[1], n_paths=n_paths, mode=mode, seed=seed, flags=flags)


@functools.lru_cache(maxsize=None)
def _rx_singles(mode, seed, n_paths):
    """every path of the receive launch of n_paths paths rendered alone, once per mode, seed and length: a shorter launch is a prefix"""
    return cr.single_path_hists(_rx(), _rx_launch(n_paths, mode, seed))


@functools.lru_cache(maxsize=None)
def _rx_expected(name, n_paths=N, mode=RAW, seed=5):
    return rr.expected(_rx(), _rx_launch(n_paths, mode, seed), table(name), _tw(), twin=_twin(), singles=_rx_singles(mode, seed, n_paths))


def _populated(exp, key=None):
    """nothing is vacuous: every bin holds paths, and so do the class outside and the miss class"""
    pop = exp.population()
    assert pop[:-2].min() >= 1 and pop[-2] > 0 and pop[-1] > 0 and pop.sum() == len(exp.cls), pop
    if key is not None:
        assert (pop[:-2].tolist(), int(pop[-2]), int(pop[-1])) == POPULATIONS[key], (key, pop)
    return pop


def _class_sums_equal_plain(h, h0, exp, lp, add, what):
    """the blocks add up to the plain histogram within two fp32 summation bounds; the count channels (A and W) exactly"""
    total = capi.split_classes(h, lp, exp.n_classes).astype(np.float64).sum(0)
    assert_two_fp32_sums(total, h0, add.S, add.N, what, counts=exp.counts)


@pytest.mark.parametrize("mode", [RAW, IQ], ids=["raw", "iq"])
def test_receive(hiplib, mode):
    sd, lp = _rx(), _rx_launch(mode=mode)
    exp, rec_o, add = _rx_expected("narrow", mode=mode)
    pop = _populated(exp, ("receive", "narrow"))
    g = capi.Scene(sd)
    h0, _, s0 = g.render(lp)
    assert g.set_range_rate_classes(table("narrow"), _tw()) == 10
    assert g.channels(lp) == 64 * 3 and g.channels(cr.classed(lp)) == 10 * 64 * 3
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and not st.kernel_variant & capi.BF_VARIANT_LEAN and not s0.kernel_variant & capi.BF_VARIANT_CLASS
    assert st.n_invalid == OracleScene(sd).render(lp)[2].n_invalid
    exp.check(h, f"receive mode {mode}, 8 bins")
    blocks = capi.split_classes(h, lp, 10)
    assert np.array_equal(blocks.reshape(10, -1, 3)[:, :, 2].sum(1), pop)          # W: one per path, in its class
    # paths whose first scatterer moves at a rate inside the window return something, and in the cells the oracle says
    live = exp.N[:8].reshape(8, -1, 3)[:, :, 0] > 0
    assert live.any() and np.array_equal(blocks[:8].reshape(8, -1, 3)[:, :, 0] != 0, live)
    _class_sums_equal_plain(h, h0, exp, lp, add, f"receive mode {mode} against the plain render")
    if mode == RAW:
        for extra, route in ((capi.BF_FLAG_GLOBAL_ATOMICS, "global atomics"), (capi.BF_FLAG_MEGAKERNEL, "one-kernel variant")):
            hr, rr_, sr = g.render(cr.classed(lp, extra), records=True)
            _same_records(rr_, rec_o)
            assert sr.kernel_variant & capi.BF_VARIANT_CLASS
            exp.check(hr, route)
            exp.check_two(hr, h, f"{route} against the default route")


def test_regeneration_and_tail(hiplib, monkeypatch):
    """1024 slots for 4096 + 37 paths: freed slots are regenerated into (the class must be the new path's, not the one the slot's
    previous path left: a path that misses after a path that hit), and the tail kernel finishes what the shade / trace iterations
    leave"""
    ragged = N + 37
    lp = _rx_launch(ragged)
    exp, rec_o, _ = rr.expected(_rx(), lp, table("narrow"), _tw(), twin=_twin(), singles=cr.single_path_hists(_rx(), lp))
    with monkeypatch.context() as m:
        m.setenv("BF_WF_POOL", "1024")
        g = capi.Scene(_rx())                # (the tunables are read when the scene is created)
    g.set_range_rate_classes(table("narrow"), _tw())
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and st.n_paths == ragged and st.n_bounces_tail > 0
    exp.check(h, "pool of 1024 slots")
    # the same launch on the default pool: every path has a slot of its own
    d = capi.Scene(_rx())
    d.set_range_rate_classes(table("narrow"), _tw())
    exp.check_two(h, d.render(cr.classed(lp))[0], "pool of 1024 slots against the default pool")


@pytest.mark.parametrize("wide", [False, True], ids=["box", "gaussian"])
def test_film(hiplib, wide):
    sd, lp = cr.film_scene()
    if wide:
        sd.sensor.rfilter = oracle_rfilter("gaussian", 0.6, block_size=4)
        sd.finalize()
    b, tw = table("film"), twists(sd)
    exp, rec_o, add = rr.expected(sd, lp, b, tw)
    _populated(exp, ("film", "film"))
    if wide:
        assert len(exp.counts) == 0      # the count channels' addends are weights
    g = capi.Scene(sd)
    assert g.set_range_rate_classes(b, tw) == 8
    assert g.channels(cr.classed(lp)) == 8 * 48 * (5 + 64)
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and bool(st.kernel_variant & capi.BF_VARIANT_WIDE) == wide
    exp.check(h, f"8 x 6 film, wide {wide}")
    hg, _, _ = g.render(cr.classed(lp, capi.BF_FLAG_GLOBAL_ATOMICS))
    exp.check(hg, f"8 x 6 film, wide {wide}, global atomics")
    _class_sums_equal_plain(h, g.render(lp)[0], exp, lp, add, f"film, wide {wide}, against the plain render")


def test_global_histogram_route(hiplib):
    """2560 range bins: 2565 floats fit the LDS, nine classes of them (23085 > kMaxLdsHist = 12288) do not, so the histogram is
    global and the base channels go through the workgroup's class table"""
    sd, lp = scenes.bus_radar(n_tris=2000, n_paths=N, bins=2560, dr=0.01, seed=7)
    b, tw = table("global"), twists(sd)
    exp, rec_o, add = rr.expected(sd, lp, b, tw)
    _populated(exp, ("global", "global"))
    g = capi.Scene(sd)
    assert g.set_range_rate_classes(b, tw) == 9
    assert g.channels(lp) == 2565 and g.channels(cr.classed(lp)) == 23085
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS
    exp.check(h, "2560 bins x 9 classes")
    _class_sums_equal_plain(h, g.render(lp)[0], exp, lp, add, "2560 bins x 9 classes against the plain render")


def test_seeded_batch(hiplib):
    seeds = [5, 31, 32]
    lp = _rx_launch(NB)
    g = capi.Scene(_rx())
    g.set_range_rate_classes(table("narrow"), _tw())
    hb, rb, st = g.render_batch(cr.classed(lp), 3, seeds=seeds, records=True)
    assert hb.shape == (3, 10 * 64 * 3) and st.kernel_variant & capi.BF_VARIANT_CLASS
    for k, seed in enumerate(seeds):
        exp, rec_o, _ = _rx_expected("narrow", NB, RAW, seed)
        _same_records(rb[k], rec_o)
        exp.check(hb[k], f"batch render {k}")
        hk, rk, _ = g.render(cr.classed(copy_launch(lp, seed=seed)), records=True)
        _same_records(rk, rec_o)
        exp.check_two(hb[k], hk, f"batch render {k} against its stand-alone render")
    assert not np.array_equal(_rx_expected("narrow", NB, RAW, 31)[0].cls, _rx_expected("narrow", NB, RAW, 32)[0].cls)


def _mesh_vertices(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()


def test_mesh_offset_batch(hiplib):
    """every mesh of render k at fl(v + offset_k): p is the shifted point, so the bus's rates move with its lever arm about the
    (world-space, unmoved) pivot, and with them the classes"""
    sd, lp = _rx(), _rx_launch(NB)
    offsets = np.array([[0.0, 0.0, 0.0], [0.5, -0.25, 0.0]], np.float32)
    g = capi.Scene(sd)
    g.set_range_rate_classes(table("narrow"), _tw())
    hb, rb, st = g.render_batch(cr.classed(lp), 2, offsets=offsets, records=True)
    assert hb.shape == (2, 10 * 64 * 3) and st.kernel_variant & capi.BF_VARIANT_CLASS
    want = motion.deformed_description(sd, {3: (_mesh_vertices(sd, 3) + offsets[1][None, :]).astype(np.float32)})
    exps = [_rx_expected("narrow", NB), rr.expected(sd, lp, table("narrow"), _tw(), twin=_twin(), trace_sd=want)]
    for k in range(2):
        _same_records(rb[k], exps[k][1])
        exps[k][0].check(hb[k], f"offset batch render {k}")
    assert not np.array_equal(exps[0][0].cls, exps[1][0].cls)


def test_motion_batch(hiplib):
    """two poses of the bus: the class is taken at the posed point.  Paths that meet the bus in both poses, on the same ray, change
    bins with the lever arm; the table (world-space twists) is the same for both renders"""
    sd, lp = _rx(), _rx_launch(NB)
    xf = np.tile(motion.rigid(), (2, len(sd.shapes), 1, 1)).astype(np.float32)
    xf[1, 3] = motion.rigid(t=(-2.0, -1.0, 0.0))
    g = capi.Scene(sd)
    g.set_range_rate_classes(table("narrow"), _tw())
    hb, rb, st = g.render_motion_batch(cr.classed(lp), xf, records=True)
    assert hb.shape == (2, 10 * 64 * 3) and st.kernel_variant & capi.BF_VARIANT_CLASS
    moved = motion.moved_description(sd, xf[1])
    exps = [_rx_expected("narrow", NB), rr.expected(sd, lp, table("narrow"), _tw(), twin=_twin(), trace_sd=moved)]
    for k in range(2):
        _same_records(rb[k], exps[k][1])
        exps[k][0].check(hb[k], f"motion batch render {k}")
    assert not np.array_equal(exps[0][1]["valid"], exps[1][1]["valid"]) and not np.array_equal(exps[0][0].cls, exps[1][0].cls)
    # the handle's own geometry and table are as they were
    _rx_expected("narrow", NB)[0].check(g.render(cr.classed(lp))[0], "after the motion batch")


def test_merged_bins(hiplib):
    """16 bins over [-8, 0) m/s (sr = 2), merged in pairs, against the device's 8 bins over the same window (sr = 1): both scales and
    every bin edge are exact, so bin k of the coarse table is bins 2k and 2k + 1 of the fine one, path for path"""
    lp = _rx_launch()
    exp, _, _ = _rx_expected("wide")
    _populated(exp, ("receive", "wide"))
    g = capi.Scene(_rx())
    assert g.set_range_rate_classes(table("wide"), _tw()) == 18
    exp.check(g.render(cr.classed(lp))[0], "16 bins")
    assert g.set_range_rate_classes(table("half"), _tw()) == 10
    assert g.channels(cr.classed(lp)) == 10 * 64 * 3
    merged = exp.merged([k // 2 for k in range(16)] + [8, 9])
    assert np.array_equal(merged.cls, _rx_expected("half")[0].cls)
    merged.check(g.render(cr.classed(lp))[0], "8 bins")


def test_one_bin_against_shape_classes(hiplib):
    """one bin over a huge window: every hit is in bin 0, nothing outside, the misses in class 2: the table
    set_classes([0] * n_shapes, 3, miss_class=2) spells out, block for block"""
    sd, lp = _rx(), _rx_launch()
    b = capi.range_rate_bins((-1e30, 1e30), 1, sensor_lin=SENSOR_LIN)
    exp, _, add = cr.expected(sd, lp, [0] * len(sd.shapes), 3, 2, twin=_twin(), singles=_rx_singles(RAW, 5, N))
    pop = exp.population()
    assert pop[0] > 0 and pop[1] == 0 and pop[2] > 0
    g = capi.Scene(sd)
    assert g.set_range_rate_classes(b, _tw()) == 3
    h = g.render(cr.classed(lp))[0]
    exp.check(h, "one bin over a huge window")
    g.set_classes([0] * len(sd.shapes), 3, 2)
    hs = g.render(cr.classed(lp))[0]
    exp.check_two(h, hs, "one bin against one shape class")      # hits and misses within two summation bounds, counts exact
    assert not capi.split_classes(h, lp, 3)[1].any() and not capi.split_classes(hs, lp, 3)[1].any()      # outside: all zeros
    assert np.array_equal(capi.split_classes(h, lp, 3).reshape(3, -1, 3)[:, :, 2].sum(1), pop)


def test_life_of_the_table(hiplib):
    import torch
    sd, lp = _rx(), _rx_launch()
    exp, rec_o, add = _rx_expected("narrow")
    by_shape = cr.expected(sd, lp, *SHAPES, twin=_twin(), singles=_rx_singles(RAW, 5, N))[0]
    by_angle = ar.expected(sd, lp, ar.bins(*ARRIVAL), twin=_twin(), singles=_rx_singles(RAW, 5, N))[0]
    g = capi.Scene(sd)
    h0 = g.render(lp)[0]
    g.set_range_rate_classes(table("narrow"), [motion.twist(**dict(zip(("lin", "ang", "pivot"), t.reshape(3, 3)))) for t in _tw()])
    h, _, st = g.render(cr.classed(lp))
    assert st.kernel_variant & capi.BF_VARIANT_CLASS
    exp.check(h, "range-rate table")
    # the blocks' count channel (W of every ADC cell) adds up to the plain render's exactly, the others within the summation bounds
    blocks = capi.split_classes(h, lp, 10).reshape(10, -1, 3)
    assert np.array_equal(blocks[:, :, 2].astype(np.float64).sum(0), h0.reshape(-1, 3)[:, 2].astype(np.float64))
    assert_two_fp32_sums(blocks.astype(np.float64).sum(0), h0, add.S, add.N, "blocks against the plain render", counts=exp.counts)
    # each of the three calls replaces another's table
    g.set_classes(*SHAPES)
    assert g.channels(cr.classed(lp)) == 4 * 64 * 3
    by_shape.check(g.render(cr.classed(lp))[0], "shape classes after a range-rate table")
    g.set_range_rate_classes(table("narrow"), _tw())
    assert g.channels(cr.classed(lp)) == 10 * 64 * 3
    exp.check(g.render(cr.classed(lp))[0], "range-rate table after shape classes")
    assert g.set_arrival_classes(ar.bins(*ARRIVAL)) == 33
    by_angle.check(g.render(cr.classed(lp))[0], "arrival table after a range-rate table")
    g.set_range_rate_classes(table("narrow"), _tw())
    exp.check(g.render(cr.classed(lp))[0], "range-rate table after an arrival table")
    # new twists under the same bins: the table is the twists' too
    g.set_range_rate_classes(table("narrow"), rr.still(sd))
    still = rr.expected(sd, lp, table("narrow"), rr.still(sd), twin=_twin(), singles=_rx_singles(RAW, 5, N))[0]
    assert not np.array_equal(still.cls, exp.cls)
    still.check(g.render(cr.classed(lp))[0], "every shape at rest")
    g.set_range_rate_classes(table("narrow"), _tw())
    # two renders on one stream with a new table between them: it takes effect for the second only
    stream = torch.cuda.Stream()
    buf = torch.zeros((2, 10 * 64 * 3), dtype=torch.float32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g.render_device(cr.classed(lp), buf[0].data_ptr(), stream=stream.cuda_stream)
    g.set_classes(*SHAPES, stream=stream.cuda_stream)
    g.render_device(cr.classed(lp), buf[1].data_ptr(), stream=stream.cuda_stream)
    g.set_range_rate_classes(table("narrow"), _tw(), stream=stream.cuda_stream)
    stream.synchronize()
    both = buf.cpu().numpy()
    exp.check(both[0], "before the shape table")
    by_shape.check(both[1][:4 * 64 * 3], "after the shape table")
    assert not both[1][4 * 64 * 3:].any()
    # a clone carries the table, as its own copy
    c = g.clone()
    assert c.channels(cr.classed(lp)) == 10 * 64 * 3
    exp.check(c.render(cr.classed(lp))[0], "clone")
    c.set_classes(*SHAPES)
    exp.check(g.render(cr.classed(lp))[0], "the original after its clone changed tables")
    c.close()
    # endpoint updates, mesh transforms and rebuilds leave it alone (world-space twists: nothing follows the meshes)
    g.update_endpoints(sd)
    g.transform_meshes(np.tile(motion.rigid(), (len(sd.shapes), 1, 1)).astype(np.float32))
    g.rebuild_bvh()
    h, rec, _ = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    exp.check(h, "after update_endpoints, transform_meshes and rebuild_bvh")
    # set_classes(n_classes = 0) clears it: the flag has nothing to split by
    g.clear_classes()
    assert g.channels(cr.classed(lp)) == g.channels(lp) == 64 * 3
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_CLASSES.*no class table"):
        g.render(cr.classed(lp))
    assert_two_fp32_sums(g.render(lp)[0], h0, add.S, add.N, "plain render after clear_classes", counts=cr.count_channels(lp))


def _status(lib, fn, *args):
    st = fn(*args)
    return st, (lib.bf_last_error() or b"").decode()


def test_refusals(hiplib):
    import torch
    lib = hiplib
    sd, lp = _rx(), _rx_launch()
    g = capi.Scene(sd)
    INVALID, UNSUPPORTED = capi.BF_ERR_INVALID, capi.BF_ERR_UNSUPPORTED
    # bf_scene_set_range_rate_classes
    nan, inf, tiny = float("nan"), float("inf"), float(np.float32(1e-45))
    ok = dict(window=(-6.0, -2.0), n_bins=8, sensor_lin=SENSOR_LIN)
    tw = capi.range_rate_twists(_tw())
    for change, message in ((dict(n_bins=0), "at least 1"), (dict(n_bins=254), None), (dict(n_bins=255), "BF_MAX_CLASSES"),
                            (dict(n_bins=0xffffffff), "BF_MAX_CLASSES"), (dict(sensor_lin=(0.0, nan, 0.0)), "sensor_lin component is not finite"),
                            (dict(sensor_lin=(inf, 0.0, 0.0)), "sensor_lin component is not finite"),
                            (dict(window=(-6.0, inf)), "window edge is not finite"), (dict(window=(nan, -2.0)), "window edge is not finite"),
                            (dict(window=(-2.0, -2.0)), "is empty"), (dict(window=(-2.0, -6.0)), "is empty"), (dict(window=(0.0, tiny)), "scale"),
                            (dict(window=(-tiny, 0.0)), "scale")):
        b = capi.range_rate_bins(**dict(ok, **change))
        st, msg = _status(lib, lib.bf_scene_set_range_rate_classes, g.handle, C.byref(b), tw.ctypes.data_as(C.c_void_p), None)
        if message is None:
            assert st == 0, (change, st, msg)
        else:
            assert st == INVALID and "bf_scene_set_range_rate_classes" in msg and message in msg, (change, st, msg)
    b = capi.range_rate_bins(**ok)
    for k, col, bad in ((3, 0, nan), (0, 4, inf), (2, 8, -inf), (1, 5, nan)):
        broken = tw.copy()
        broken[k, col] = bad
        st, msg = _status(lib, lib.bf_scene_set_range_rate_classes, g.handle, C.byref(b), broken.ctypes.data_as(C.c_void_p), None)
        assert st == INVALID and f"bf_scene_set_range_rate_classes: twists[{k}]" in msg and "not finite" in msg, (k, col, st, msg)
    st, msg = _status(lib, lib.bf_scene_set_range_rate_classes, g.handle, None, tw.ctypes.data_as(C.c_void_p), None)
    assert st == INVALID and "bf_scene_set_range_rate_classes: null bins" in msg, (st, msg)
    st, msg = _status(lib, lib.bf_scene_set_range_rate_classes, g.handle, C.byref(b), None, None)
    assert st == INVALID and "bf_scene_set_range_rate_classes: twists is null" in msg, (st, msg)
    with pytest.raises(ValueError, match="3 twists for a scene of 4 shapes"):
        g.set_range_rate_classes(b, _tw()[:3])
    g.clear_classes()
    # a refused table installs nothing: the flag without a table
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_CLASSES.*no class table"):
        g.render(cr.classed(lp))
    g.set_range_rate_classes(table("narrow"), _tw())
    # everything shape classes are refused for, with the same status and message
    for extra, name in ((capi.BF_FLAG_FAST, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, "BF_FLAG_MOMENT")):
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_CLASSES.*{name}"):
            g.render(cr.classed(lp, extra))
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM with BF_FLAG_CLASSES"):
        g.render(cr.classed(lp, capi.BF_FLAG_EXACT_SUM))
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        capi.render_sharded([g], cr.classed(lp))
    buf = torch.zeros(10 * 64 * 3, dtype=torch.float32, device="cuda")
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        capi.render_sharded_device([g], cr.classed(lp), [buf.data_ptr()])
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        g.render_converge(cr.classed(lp), 0.1, max_rounds=2)
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        g.render_converge_device(cr.classed(lp), buf.data_ptr(), 0.1, max_rounds=2)
    # the motion batch entry refuses before it prepares anything
    xf = np.tile(motion.rigid(), (2, len(sd.shapes), 1, 1)).astype(np.float32)
    for extra, name in ((capi.BF_FLAG_FAST, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, "BF_FLAG_MOMENT")):
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_CLASSES.*{name}"):
            g.render_motion_batch(cr.classed(lp, extra), xf)
    # AOVs (a render mode: the film scene)
    fd, fl = cr.film_scene()
    f = capi.Scene(fd)
    f.set_aovs(["depth"])
    f.set_range_rate_classes(table("film"), twists(fd))
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_AOV.*BF_FLAG_CLASSES"):
        f.render(cr.classed(fl, capi.BF_FLAG_AOV))
    f.close()
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
        assert_fp32_sum(h[k], add.ref, add.S, add.N, f"rolling render {k} around the refusal", counts=cr.count_channels(lp))
    # the handle is usable and the table survived all of it
    _rx_expected("narrow")[0].check(g.render(cr.classed(lp))[0], "after the refusals")


def test_motion_sweep_with_range_rate_bins(hiplib):
    """4 pulses of the bus driving off: the cube gains the class axis behind the pulse axis; pulse 0 (the scene as described) is the
    stand-alone classed render"""
    from beifong_amd import sweep
    sd, lp = _rx(), _rx_launch(NB)
    n_pulses = 4
    xf = np.tile(motion.rigid(), (n_pulses, len(sd.shapes), 1, 1)).astype(np.float32)
    xf[:, 3, 0, 3] = 0.25 * np.arange(n_pulses)
    cube = sweep.render_motion_sweep(sd, lp, xf, n_streams=2, classes=(table("narrow"), _tw()))
    plain = sweep.render_motion_sweep(sd, lp, xf, n_streams=2)
    assert cube.shape == (n_pulses, 10, 64, 3) and plain.shape == (n_pulses, 64, 3)
    assert sweep.range_doppler(cube[:, 7]).shape == (n_pulses, 64)
    assert np.array_equal(cube[..., 2].sum(1), plain[..., 2])                   # W: exact
    exp = _rx_expected("narrow", NB)[0]
    g = capi.Scene(sd)
    g.set_range_rate_classes(table("narrow"), _tw())
    exp.check_two(cube[0], g.render(cr.classed(lp))[0], "pulse 0 against the stand-alone classed render")
    exp.check(cube[0], "pulse 0")


def test_range_rate_bins_are_the_sweeps_doppler_rows(hiplib):
    """The new axis against the coherent one.  Two plates step dx_i per pulse (range_rate_ref.two_plates, the scene of the two-target
    motion sweeps of tests/test_gpu_motion.py and tests/test_gpu_motion_batch.py; such a sweep of n_pulses pulses finds plate i's line in FFT row round(2 |dx_i| / lambda * n_pulses) mod n_pulses).  With a pulse repetition
    interval T that step is the velocity dx_i / T, and n_pulses bins over the unambiguous span [-lambda / 4T, lambda / 4T) are as
    wide as one FFT row: bin k holds the rates whose Doppler shift -2 rr / lambda, in rows of 1 / (n_pulses T), lies in
    (n_pulses / 2 - k - 1, n_pulses / 2 - k], its centre at row n_pulses / 2 - k - 1/2.  A plate seen along d closes at dx_i d.x / T
    with d.x in (0.96, 1], so ONE classed render puts plate i's paths in a bin whose centre's row, rounded, is within one row of
    the sweep's; the ground and the apertures, at rest, are in row 0's."""
    lam, n_pulses, T = 0.1, 64, 1.0e-3
    dx = (-0.004, -0.0125)
    sd, lp, plates = rr.two_plates()
    lp = copy_launch(lp, n_paths=1 << 14)
    span = lam / (4.0 * T)
    b = capi.range_rate_bins((-span, span), n_pulses)
    tw = rr.still(sd)
    for i, k in enumerate(plates):
        tw[k] = motion.twist(lin=(dx[i] / T, 0.0, 0.0))
    g = capi.Scene(sd)
    assert g.set_range_rate_classes(b, tw) == n_pulses + 2
    h = g.render(cr.classed(lp))[0]
    pop = capi.split_classes(h, lp, n_pulses + 2).reshape(n_pulses + 2, -1, 3)[:, :, 2].sum(1)      # W: the paths of every class
    assert pop.sum() == lp.n_paths and pop[n_pulses] == 0
    rows = np.asarray([int(round(-2.0 * c * T * n_pulses / lam)) % n_pulses for c in capi.range_rate_centres(b)])
    assert np.allclose(-2.0 * capi.range_rate_centres(b) * T * n_pulses / lam, n_pulses / 2 - np.arange(n_pulses) - 0.5, rtol=0, atol=1e-9)
    # the same paths by the shape they meet first
    shape_class = np.zeros(len(sd.shapes), np.uint32)
    shape_class[plates[0]], shape_class[plates[1]] = 1, 2
    g.set_classes(shape_class, 4, 3)
    by_shape = capi.split_classes(g.render(cr.classed(lp))[0], lp, 4).reshape(4, -1, 3)[:, :, 2].sum(1)
    assert by_shape[1] > 0 and by_shape[2] > 0 and by_shape[3] == pop[n_pulses + 1]
    near = lambda row, want: min((row - want) % n_pulses, (want - row) % n_pulses) <= 1
    expect = [int(round(2 * abs(dx[i]) / lam * n_pulses)) % n_pulses for i in range(2)]
    assert expect == [5, 16]
    populated = np.flatnonzero(pop[:n_pulses])
    for i in range(2):
        mine = [k for k in populated if near(rows[k], expect[i])]
        assert mine and pop[mine].sum() == by_shape[1 + i], (i, mine, pop[mine], by_shape)
    at_rest = [k for k in populated if near(rows[k], 0)]
    assert pop[at_rest].sum() == by_shape[0]
    assert all(near(rows[k], 0) or near(rows[k], expect[0]) or near(rows[k], expect[1]) for k in populated), (populated, rows[populated])
