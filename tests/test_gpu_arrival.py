"""Returns by direction of arrival (Scene.set_arrival_classes with BF_FLAG_CLASSES): the class of a path is the bin of
its primary ray's direction.  Expected cells come from the unchanged oracle through tests/arrival_ref.py (the direction of every
path's composed primary ray -> capi.arrival_classes -> class_ref.per_class: every path rendered alone).  Every block of every
device histogram is held to its per-cell fp32 summation bound; unpopulated cells are exactly zero, the count channels exact per
class, and the per-path records bit-equal to the oracle's."""
import ctypes as C
import functools

import numpy as np
import pytest

from beifong_amd import capi, motion, scenes
from tests import arrival_ref as ar
from tests import class_ref as cr
from tests.hist_bound import assert_fp32_sum, assert_two_fp32_sums
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _same_records
from tests.scene_builders import oracle_rfilter

pytestmark = pytest.mark.gpu

N, NB = 4096, 1024           # paths of a single render; of every render of a batch
RAW, IQ = capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ
CLS = capi.BF_FLAG_CLASSES
TABLES = {
    "narrow": (8, 4, (0.0, 0.6, -0.2, 0.4)),          # most paths arrive from outside
    "sphere": (8, 4, (-1.0, 1.0, -1.0, 1.0)),         # every direction is inside
    "row": (8, 1, (-1.0, 1.0, -2.0, 2.0)),            # "sphere" with its v bins merged
    "film": (6, 4, (-0.3, 0.3, -0.2, 0.2)),
    "wide": (4, 2, (-0.3, 0.3, -0.3, 0.3)),
}
SHAPES = ([0, 0, 1, 2], 4, 3)      # the receive scene by shape: both apertures, ground, bus, miss


def _table(name):
    return ar.bins(*TABLES[name])


@functools.lru_cache(maxsize=None)
def _rx():
    return cr.receive_scene(N)[0]


@functools.lru_cache(maxsize=None)
def _twin():
    return cr.fluxmeter_twin(cr.receive_scene)


def _rx_launch(n_paths=N, mode=RAW, seed=5, flags=0):
    return copy_launch(cr.receive_scene(N)[1], n_paths=n_paths, mode=mode, seed=seed, flags=flags)


@functools.lru_cache(maxsize=None)
def _rx_singles(mode, seed):
    """every path of the receive launch rendered alone, once per mode and seed: a shorter launch is a prefix"""
    return cr.single_path_hists(_rx(), _rx_launch(N if seed == 5 else NB, mode, seed))


@functools.lru_cache(maxsize=None)
def _rx_expected(name, n_paths=N, mode=RAW, seed=5):
    return ar.expected(_rx(), _rx_launch(n_paths, mode, seed), _table(name), twin=_twin(), singles=_rx_singles(mode, seed))


def _populated(exp, narrow):
    """nothing is vacuous: every bin holds paths and, where the window is narrow, so does the class outside"""
    pop = exp.population()
    assert pop[:-1].min() >= 1 and pop.sum() == len(exp.cls) and (pop[-1] > 0) == narrow, pop
    return pop


def _class_sums_equal_plain(h, h0, exp, lp, add, what):
    """the blocks add up to the plain histogram within two fp32 summation bounds; the count channels (A and W) exactly"""
    total = capi.split_classes(h, lp, exp.n_classes).astype(np.float64).sum(0)
    assert_two_fp32_sums(total, h0, add.S, add.N, what, counts=exp.counts)


@pytest.mark.parametrize("mode", [RAW, IQ], ids=["raw", "iq"])
def test_receive(hiplib, mode):
    sd, lp = _rx(), _rx_launch(mode=mode)
    exp, rec_o, add = _rx_expected("narrow", mode=mode)
    pop = _populated(exp, True)
    g = capi.Scene(sd)
    h0, _, s0 = g.render(lp)
    assert g.set_arrival_classes(_table("narrow")) == 33
    assert g.channels(lp) == 64 * 3 and g.channels(cr.classed(lp)) == 33 * 64 * 3
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and not st.kernel_variant & capi.BF_VARIANT_LEAN and not s0.kernel_variant & capi.BF_VARIANT_CLASS
    assert st.n_invalid == OracleScene(sd).render(lp)[2].n_invalid
    exp.check(h, f"receive mode {mode}, 8 x 4 bins")
    blocks = capi.split_classes(h, lp, 33)
    assert np.array_equal(blocks.reshape(33, -1, 3)[:, :, 2].sum(1), pop)          # W: one per path, in its class
    # paths that arrive through the window return something, and in the cells the oracle says
    live = exp.N[:32].reshape(32, -1, 3)[:, :, 0] > 0
    assert live.any() and np.array_equal(blocks[:32].reshape(32, -1, 3)[:, :, 0] != 0, live)
    _class_sums_equal_plain(h, h0, exp, lp, add, f"receive mode {mode} against the plain render")
    if mode == RAW:
        for extra, route in ((capi.BF_FLAG_GLOBAL_ATOMICS, "global atomics"), (capi.BF_FLAG_MEGAKERNEL, "one-kernel variant")):
            hr, rr, sr = g.render(cr.classed(lp, extra), records=True)
            _same_records(rr, rec_o)
            assert sr.kernel_variant & capi.BF_VARIANT_CLASS
            exp.check(hr, route)
            exp.check_two(hr, h, f"{route} against the default route")


def test_regeneration_and_tail(hiplib, monkeypatch):
    """1024 slots for 4096 + 37 paths: freed slots are regenerated into (the class must be the new path's, not the one the slot's
    previous path left), and the tail kernel finishes what the shade / trace iterations leave"""
    ragged = N + 37
    lp = _rx_launch(ragged)
    exp, rec_o, _ = ar.expected(_rx(), lp, _table("narrow"), twin=_twin(), singles=cr.single_path_hists(_rx(), lp))
    with monkeypatch.context() as m:
        m.setenv("BF_WF_POOL", "1024")
        g = capi.Scene(_rx())                # (the tunables are read when the scene is created)
    g.set_arrival_classes(_table("narrow"))
    h, rec, st = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and st.n_paths == ragged and st.n_bounces_tail > 0
    exp.check(h, "pool of 1024 slots")
    # the same launch on the default pool: every path has a slot of its own
    d = capi.Scene(_rx())
    d.set_arrival_classes(_table("narrow"))
    exp.check_two(h, d.render(cr.classed(lp))[0], "pool of 1024 slots against the default pool")


@pytest.mark.parametrize("wide", [False, True], ids=["box", "gaussian"])
def test_film(hiplib, wide):
    sd, lp = cr.film_scene()
    if wide:
        sd.sensor.rfilter = oracle_rfilter("gaussian", 0.6, block_size=4)
        sd.finalize()
    table = _table("film")
    exp, rec_o, add = ar.expected(sd, lp, table)
    _populated(exp, True)
    if wide:
        assert len(exp.counts) == 0      # the count channels' addends are weights
    g = capi.Scene(sd)
    assert g.set_arrival_classes(table) == 25
    assert g.channels(cr.classed(lp)) == 25 * 48 * (5 + 64)
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
    table = _table("wide")
    exp, rec_o, add = ar.expected(sd, lp, table)
    _populated(exp, True)
    g = capi.Scene(sd)
    g.set_arrival_classes(table)
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
    g.set_arrival_classes(_table("narrow"))
    hb, rb, st = g.render_batch(cr.classed(lp), 3, seeds=seeds, records=True)
    assert hb.shape == (3, 33 * 64 * 3) and st.kernel_variant & capi.BF_VARIANT_CLASS
    for k, seed in enumerate(seeds):
        exp, rec_o, _ = _rx_expected("narrow", NB, RAW, seed)
        _same_records(rb[k], rec_o)
        exp.check(hb[k], f"batch render {k}")
        hk, rk, _ = g.render(cr.classed(copy_launch(lp, seed=seed)), records=True)
        _same_records(rk, rec_o)
        exp.check_two(hb[k], hk, f"batch render {k} against its stand-alone render")
    assert not np.array_equal(_rx_expected("narrow", NB, RAW, 31)[0].cls, _rx_expected("narrow", NB, RAW, 32)[0].cls)


def test_motion_batch(hiplib):
    """two poses of the bus: the class depends on the ray alone, so both renders have the same class vector, and different returns"""
    sd, lp = _rx(), _rx_launch(NB)
    xf = np.tile(motion.rigid(), (2, len(sd.shapes), 1, 1)).astype(np.float32)
    xf[1, 3] = motion.rigid(t=(-2.0, -1.0, 0.0))
    g = capi.Scene(sd)
    g.set_arrival_classes(_table("narrow"))
    hb, rb, st = g.render_motion_batch(cr.classed(lp), xf, records=True)
    assert hb.shape == (2, 33 * 64 * 3) and st.kernel_variant & capi.BF_VARIANT_CLASS
    exps = [_rx_expected("narrow", NB)[0], ar.expected(sd, lp, _table("narrow"), twin=_twin(), trace_sd=motion.moved_description(sd, xf[1]))[0]]
    recs = [_rx_expected("narrow", NB)[1], OracleScene(motion.moved_description(sd, xf[1])).render(lp, records=True, threads=8)[1]]
    assert np.array_equal(exps[0].cls, exps[1].cls)
    for k in range(2):
        _same_records(rb[k], recs[k])
        exps[k].check(hb[k], f"motion batch render {k}")
    assert not np.array_equal(recs[0]["valid"], recs[1]["valid"]) and not np.array_equal(hb[0], hb[1])
    # the handle's own geometry and table are as they were
    _rx_expected("narrow", NB)[0].check(g.render(cr.classed(lp))[0], "after the motion batch")


def test_merged_bins(hiplib):
    """8 x 4 bins over the whole sphere, their v bins merged, against the device's 8 x 1 table over the same u window"""
    lp = _rx_launch()
    exp, _, _ = _rx_expected("sphere")
    _populated(exp, False)
    g = capi.Scene(_rx())
    assert g.set_arrival_classes(_table("sphere")) == 33
    exp.check(g.render(cr.classed(lp))[0], "8 x 4 bins over the sphere")
    assert g.set_arrival_classes(_table("row")) == 9
    assert g.channels(cr.classed(lp)) == 9 * 64 * 3
    exp.merged([k % 8 for k in range(32)] + [8]).check(g.render(cr.classed(lp))[0], "8 x 1 bins")


def test_life_of_the_table(hiplib):
    import torch
    sd, lp = _rx(), _rx_launch()
    exp, rec_o, add = _rx_expected("narrow")
    by_shape = cr.expected(sd, lp, *SHAPES, twin=_twin(), singles=_rx_singles(RAW, 5))[0]
    g = capi.Scene(sd)
    h0 = g.render(lp)[0]
    g.set_arrival_classes(ar.AXIS_U, ar.AXIS_V, *TABLES["narrow"])      # the five-argument form
    h, _, st = g.render(cr.classed(lp))
    assert st.kernel_variant & capi.BF_VARIANT_CLASS
    exp.check(h, "arrival table")
    # the blocks' count channel (W of every ADC cell) adds up to the plain render's exactly, the others within the summation bounds
    blocks = capi.split_classes(h, lp, 33).reshape(33, -1, 3)
    assert np.array_equal(blocks[:, :, 2].astype(np.float64).sum(0), h0.reshape(-1, 3)[:, 2].astype(np.float64))
    assert_two_fp32_sums(blocks.astype(np.float64).sum(0), h0, add.S, add.N, "blocks against the plain render", counts=exp.counts)
    # each of the two calls replaces the other's table
    g.set_classes(*SHAPES)
    assert g.channels(cr.classed(lp)) == 4 * 64 * 3
    by_shape.check(g.render(cr.classed(lp))[0], "shape classes after an arrival table")
    g.set_arrival_classes(_table("narrow"))
    assert g.channels(cr.classed(lp)) == 33 * 64 * 3
    exp.check(g.render(cr.classed(lp))[0], "arrival table after shape classes")
    # two renders on one stream with a new table between them: it takes effect for the second only
    stream = torch.cuda.Stream()
    buf = torch.zeros((2, 33 * 64 * 3), dtype=torch.float32, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    g.render_device(cr.classed(lp), buf[0].data_ptr(), stream=stream.cuda_stream)
    g.set_classes(*SHAPES, stream=stream.cuda_stream)
    g.render_device(cr.classed(lp), buf[1].data_ptr(), stream=stream.cuda_stream)
    g.set_arrival_classes(_table("narrow"), stream=stream.cuda_stream)
    stream.synchronize()
    both = buf.cpu().numpy()
    exp.check(both[0], "before the shape table")
    by_shape.check(both[1][:4 * 64 * 3], "after the shape table")
    assert not both[1][4 * 64 * 3:].any()
    # a clone carries the table, as its own copy
    c = g.clone()
    assert c.channels(cr.classed(lp)) == 33 * 64 * 3
    exp.check(c.render(cr.classed(lp))[0], "clone")
    c.set_classes(*SHAPES)
    exp.check(g.render(cr.classed(lp))[0], "the original after its clone changed tables")
    c.close()
    # endpoint updates, mesh transforms and rebuilds leave it alone (world-space axes: nothing follows the sensor)
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
    # bf_scene_set_arrival_classes
    nan, inf, tiny = float("nan"), float("inf"), float(np.float32(1e-45))
    ok = dict(axis_u=ar.AXIS_U, axis_v=ar.AXIS_V, n_u=8, n_v=4, window=(0.0, 0.6, -0.2, 0.4))
    for change, message in ((dict(n_u=0), "at least 1"), (dict(n_v=0), "at least 1"), (dict(n_u=16, n_v=16), "BF_MAX_CLASSES"),
                            (dict(n_u=255, n_v=1), None), (dict(n_u=256, n_v=1), "BF_MAX_CLASSES"), (dict(n_u=65536, n_v=65536), "BF_MAX_CLASSES"),
                            (dict(axis_u=(0.0, nan, 0.0)), "axis component is not finite"), (dict(axis_v=(inf, 0.0, 0.0)), "axis component is not finite"),
                            (dict(window=(0.0, inf, -0.2, 0.4)), "window edge is not finite"), (dict(window=(0.0, 0.6, nan, 0.4)), "window edge is not finite"),
                            (dict(window=(0.6, 0.6, -0.2, 0.4)), "is empty"), (dict(window=(0.0, 0.6, 0.4, -0.2)), "is empty"),
                            (dict(window=(0.0, tiny, -0.2, 0.4)), "scale"), (dict(window=(0.0, 0.6, -tiny, 0.0)), "scale")):
        b = capi.arrival_bins(**dict(ok, **change))
        st, msg = _status(lib, lib.bf_scene_set_arrival_classes, g.handle, C.byref(b), None)
        if message is None:
            assert st == 0, (change, st, msg)
        else:
            assert st == INVALID and "bf_scene_set_arrival_classes" in msg and message in msg, (change, st, msg)
    st, msg = _status(lib, lib.bf_scene_set_arrival_classes, g.handle, None, None)
    assert st == INVALID and "bf_scene_set_arrival_classes: null bins" in msg, (st, msg)
    g.clear_classes()
    # a refused table installs nothing: the flag without a table
    with pytest.raises(capi.BeifongError, match=r"status 1\).*BF_FLAG_CLASSES.*no class table"):
        g.render(cr.classed(lp))
    g.set_arrival_classes(_table("narrow"))
    # everything shape classes are refused for, with the same status and message
    for extra, name in ((capi.BF_FLAG_FAST, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, "BF_FLAG_MOMENT")):
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_CLASSES.*{name}"):
            g.render(cr.classed(lp, extra))
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM with BF_FLAG_CLASSES"):
        g.render(cr.classed(lp, capi.BF_FLAG_EXACT_SUM))
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_CLASSES"):
        capi.render_sharded([g], cr.classed(lp))
    buf = torch.zeros(33 * 64 * 3, dtype=torch.float32, device="cuda")
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
    f.set_arrival_classes(_table("film"))
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


def test_motion_sweep_with_arrival_bins(hiplib):
    """4 pulses of the bus driving off: the cube gains the class axis behind the pulse axis; pulse 0 (the scene as described) is the
    stand-alone classed render"""
    pytest.importorskip("torch")
    from beifong_amd import sweep
    sd, lp = _rx(), _rx_launch(NB)
    n_pulses = 4
    xf = np.tile(motion.rigid(), (n_pulses, len(sd.shapes), 1, 1)).astype(np.float32)
    xf[:, 3, 0, 3] = 0.25 * np.arange(n_pulses)
    cube = sweep.render_motion_sweep(sd, lp, xf, n_streams=2, classes=_table("narrow"))
    plain = sweep.render_motion_sweep(sd, lp, xf, n_streams=2)
    assert cube.shape == (n_pulses, 33, 64, 3) and plain.shape == (n_pulses, 64, 3)
    assert sweep.range_doppler(cube[:, 7]).shape == (n_pulses, 64)
    assert np.array_equal(cube[..., 2].sum(1), plain[..., 2])                   # W: exact
    exp = _rx_expected("narrow", NB)[0]
    g = capi.Scene(sd)
    g.set_arrival_classes(_table("narrow"))
    exp.check_two(cube[0], g.render(cr.classed(lp))[0], "pulse 0 against the stand-alone classed render")
    exp.check(cube[0], "pulse 0")
