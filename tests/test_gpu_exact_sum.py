"""Exact-sum renders (BF_FLAG_EXACT_SUM): every histogram cell is fl(sum of its addends), one rounding.

1. the probe bf_exact_sum (the device functions the kSum kernels add with, and their resolve kernel) against the specification
   capi.exact_sum, bit for bit, on the adversarial sets of tests/exact_sum_sets.py, on 2^25 unit addends and on random ones;
2. renders against capi.exact_sum over the oracle's single-path histograms (class_ref.single_path_hists: a path gives a cell at
   most one addend), array_equal on the bit patterns;
3. one launch, one answer: every route, twice, batches against their stand-alone renders;
4. kernel_variant and the refusals.

EXCLUDED names the kinds of addend that are NOT held to the oracle bit for bit (DESIGN.md 6j has the finding); at most the two
kinds existing parity tests never proved: addends that pass through srgb_to_xyz_grey, addends multiplied by a filter weight.  Their
cells keep the per-cell bound of hist_bound.assert_fp32_sum, and test 3 covers them like every other cell."""
import functools

import numpy as np
import pytest

from beifong_amd import capi, motion, scenes
from tests import class_ref as cr
from tests import exact_sum_sets as sets
from tests.hist_bound import assert_fp32_sum
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _same_records
from tests.scene_builders import oracle_rfilter

pytestmark = pytest.mark.gpu

SUM = capi.BF_FLAG_EXACT_SUM
N, BINS, SPAN = 4096, 64, 25.6
RAGGED = N + 37
SRGB, FILTERED = "srgb_to_xyz_grey", "filter_weight"
EXCLUDED = ()      # of (SRGB, FILTERED)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def summed(lp, extra=0, **kw):
    return copy_launch(lp, flags=lp.flags | SUM | extra, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the probe
# ---------------------------------------------------------------------------------------------------------------------------------
ALL_SETS = sets.sets()


@pytest.mark.parametrize("in_lds", [0, 1], ids=["global", "lds"])
@pytest.mark.parametrize("name,cell,value,n_cells", ALL_SETS, ids=[s[0] for s in ALL_SETS])
def test_probe_adversarial_sets(hiplib, name, cell, value, n_cells, in_lds):
    want = capi.exact_sum(cell, value, n_cells)
    for k, (c, v) in enumerate(sets.shuffles(cell, value)):
        got = capi.exact_sum_device(c, v, n_cells, in_lds, hiplib)
        assert np.array_equal(bits(got), bits(want)), (name, in_lds, k, got, want)


@pytest.mark.parametrize("in_lds", [0, 1], ids=["global", "lds"])
def test_probe_counts_past_2_24(hiplib, in_lds):
    """what the feature buys: an fp32 atomic sum of ones stops at 16777216"""
    n = 1 << 25
    got = capi.exact_sum_device(np.zeros(n, np.uint32), np.ones(n, np.float32), 1, in_lds, hiplib)
    assert got[0] == 33554432.0


@pytest.mark.parametrize("in_lds", [0, 1], ids=["global", "lds"])
@pytest.mark.parametrize("n_cells", [3, 4097])      # (4097 cells do not fit the LDS: global limbs by size, as in a render)
def test_probe_random_addends(hiplib, n_cells, in_lds):
    rng = np.random.default_rng(n_cells)
    value = sets.random_bits(rng, 1 << 20, None)
    # moderate exponents as well: uniformly random exponents leave the sum to the few largest addends
    value[::2] = (rng.standard_normal(value[::2].size) * 10.0 ** rng.integers(-3, 4, value[::2].size)).astype(np.float32)
    cell = rng.integers(0, n_cells, size=value.size).astype(np.uint32)
    want = capi.exact_sum(cell, value, n_cells)
    got = capi.exact_sum_device(cell, value, n_cells, in_lds, hiplib)
    assert np.array_equal(bits(got), bits(want))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. renders equal the exactly rounded oracle sum
# ---------------------------------------------------------------------------------------------------------------------------------
class Exact(object):
    """the expectation of one launch from its single-path histograms: fl(sum) per cell, N, and ref / S for the excluded kinds"""

    def __init__(self, singles, n_paths, n_chan):
        cells = np.concatenate([singles[p][0] for p in range(n_paths)]).astype(np.uint32)
        vals64 = np.concatenate([singles[p][1] for p in range(n_paths)])
        self.cells, self.vals = cells, vals64.astype(np.float32)
        assert np.array_equal(self.vals.astype(np.float64), vals64)
        self.want = capi.exact_sum(cells, self.vals, n_chan)
        self.N = np.bincount(cells, minlength=n_chan)
        self.ref, self.S = np.zeros(n_chan), np.zeros(n_chan)
        np.add.at(self.ref, cells, vals64)
        np.add.at(self.S, cells, np.abs(vals64))


def kind_masks(lp, n_chan, wide):
    """which cells of the launch's histogram take addends of the two unproven kinds, from the layout alone (include/beifong_hip.h)"""
    srgb = np.zeros(n_chan, bool)
    render_mode = lp.mode in (capi.BF_MODE_PATH, capi.BF_MODE_RANGE, capi.BF_MODE_TIME)
    if render_mode and lp.color_mode == capi.BF_COLOR_RGB:
        px = lp.film_width * lp.film_height if (lp.spp and lp.film_width and lp.film_height) else 1
        per = srgb.reshape(px, n_chan // px)
        per[:, 0:3] = True                                  # X Y Z
        if lp.mode == capi.BF_MODE_TIME:
            per[:, 5:] = True                               # S{i}.R G B
    return {SRGB: srgb, FILTERED: np.full(n_chan, bool(wide))}


def check_exact(h, exp, lp, what, wide=False):
    h = np.asarray(h, np.float32).reshape(-1)
    assert h.size == exp.want.size, (what, h.size, exp.want.size)
    masks = kind_masks(lp, h.size, wide)
    excl = np.zeros(h.size, bool)
    for kind in EXCLUDED:
        excl |= masks[kind]
    diff = np.flatnonzero((bits(h) != bits(exp.want)) & ~excl)
    assert diff.size == 0, (what, diff[:8], h[diff[:8]], exp.want[diff[:8]], exp.N[diff[:8]],
                            {k: int((m[diff]).sum()) for k, m in masks.items()})
    assert not bits(h)[exp.N == 0].any(), what                # a cell without addends is exactly +0.0
    if excl.any():
        assert_fp32_sum(h[excl], exp.ref[excl], exp.S[excl], exp.N[excl], f"{what}: excluded kinds")


def _c4_launch(n_paths=N, bins=BINS, mode=capi.BF_MODE_RANGE, color=capi.BF_COLOR_RGB, seed=3, flags=0):
    return capi.make_launch(mode, n_paths, seed=seed, bins=0 if mode == capi.BF_MODE_PATH else bins, bin_width=SPAN / bins, color_mode=color,
                            flags=flags)


@functools.lru_cache(maxsize=None)
def _c4():
    return scenes.multi_mesh_radar(n_paths=N, bins=BINS, dr=SPAN / BINS, seed=3, scale=0.01)[0]


@functools.lru_cache(maxsize=None)
def _c4_singles(bins=BINS, mode=capi.BF_MODE_RANGE, color=capi.BF_COLOR_RGB):
    """the RAGGED single-path histograms of a C4 launch: every shorter launch of the same seed is a prefix"""
    return cr.single_path_hists(_c4(), _c4_launch(RAGGED, bins, mode, color))


@functools.lru_cache(maxsize=None)
def _c4_exact(n_paths=N, bins=BINS, mode=capi.BF_MODE_RANGE, color=capi.BF_COLOR_RGB):
    n_chan = 5 + (0 if mode == capi.BF_MODE_PATH else bins)
    return Exact(_c4_singles(bins, mode, color), n_paths, n_chan)


def _render_checked(g, lp, rec_o=None):
    h, rec, st = g.render(summed(lp), records=True)
    assert st.kernel_variant & capi.BF_VARIANT_EXACT_SUM and not st.kernel_variant & capi.BF_VARIANT_LEAN, st.kernel_variant
    assert st.n_paths == lp.n_paths
    if rec_o is not None:
        _same_records(rec, rec_o)      # records are unchanged
    return h


@pytest.mark.parametrize("color", [capi.BF_COLOR_RGB, capi.BF_COLOR_MONO], ids=["rgb", "mono"])
def test_c4_range_mode(hiplib, color):
    lp = _c4_launch(color=color)
    g = capi.Scene(_c4())
    rec_o = OracleScene(_c4()).render(lp, records=True, threads=8)[1]
    h = _render_checked(g, lp, rec_o)
    exp = _c4_exact(color=color)
    assert exp.N[4] == N and np.count_nonzero(exp.N[5:]) >= 6      # nothing is vacuous
    check_exact(h, exp, lp, f"C4 range mode, colour {color}")
    assert h[4] == N


def test_path_mode(hiplib):
    lp = _c4_launch(mode=capi.BF_MODE_PATH)
    h = _render_checked(capi.Scene(_c4()), lp)
    assert h.size == 5
    check_exact(h, _c4_exact(mode=capi.BF_MODE_PATH), lp, "path mode")


def test_time_mode_through_the_flux_meter(hiplib):
    sd, lp = scenes.trans_rad(spp=N)
    g = capi.Scene(sd)
    exp = Exact(cr.single_path_hists(sd, lp), N, g.channels(lp))
    check_exact(_render_checked(g, lp), exp, lp, "time mode, flux meter")
    check_exact(g.render(summed(lp, capi.BF_FLAG_MEGAKERNEL))[0], exp, lp, "time mode, one-kernel variant")


@pytest.mark.parametrize("wide", [False, True], ids=["box", "gaussian"])
def test_film(hiplib, wide):
    sd, lp = cr.film_scene()
    if wide:
        sd.sensor.rfilter = oracle_rfilter("gaussian", 0.6, block_size=4)
        sd.finalize()
    g = capi.Scene(sd)
    assert g.channels(lp) == 48 * (5 + 64)      # 3312 cells: global limbs by size
    exp = Exact(cr.single_path_hists(sd, lp), int(lp.n_paths), g.channels(lp))
    h, _, st = g.render(summed(lp))
    assert st.kernel_variant & capi.BF_VARIANT_EXACT_SUM and bool(st.kernel_variant & capi.BF_VARIANT_WIDE) == wide
    check_exact(h, exp, lp, f"8 x 6 film, wide {wide}", wide)
    hg, _, _ = g.render(summed(lp, capi.BF_FLAG_GLOBAL_ATOMICS))
    assert np.array_equal(bits(hg), bits(h))


@pytest.mark.parametrize("case", ["raw_phase_bins", "iq_adc_window"])
def test_receive_modes(hiplib, case):
    sd, lp = cr.receive_scene()
    if case == "iq_adc_window":
        sd.sensor.window_offset_t, sd.sensor.window_t_bins, sd.sensor.window_offset_f, sd.sensor.window_f_bins = 5, 40, 0, 1
        sd.finalize()
        lp.mode, lp.bins = capi.BF_MODE_RECEIVE_IQ, 40
    else:
        lp.phase_bins = 4
    g = capi.Scene(sd)
    exp = Exact(cr.single_path_hists(sd, lp), N, g.channels(lp))
    if case == "iq_adc_window":
        # the launch with signed addends (negative cells; within one cell of this launch the signs agree: cancellation inside a
        # cell is the probe's ground)
        assert (exp.vals < 0).any() and (exp.ref < 0).any()
    rec_o = OracleScene(sd).render(lp, records=True, threads=8)[1]
    check_exact(_render_checked(g, lp, rec_o), exp, lp, case)
    check_exact(g.render(summed(lp, capi.BF_FLAG_MEGAKERNEL))[0], exp, lp, f"{case}, one-kernel variant")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. one launch, one answer
# ---------------------------------------------------------------------------------------------------------------------------------
ROUTES = ["default", "no_tail", "small_pool", "megakernel", "global_atomics"]


def test_routes_of_one_launch(hiplib, monkeypatch):
    """a ragged launch (4096 + 37 paths) over five routes and twice over the first: bit-identical, and equal to the oracle's sum"""
    exp = _c4_exact(RAGGED)
    hists = {}
    for route in ROUTES:
        with monkeypatch.context() as m:
            if route == "no_tail":
                m.setenv("BF_WF_TAIL", "0")
            if route == "small_pool":
                m.setenv("BF_WF_POOL", "1024")
            g = capi.Scene(_c4())            # (after setenv: the tunables are read when the scene is created)
        lp = _c4_launch(RAGGED, flags=SUM | {"megakernel": capi.BF_FLAG_MEGAKERNEL, "global_atomics": capi.BF_FLAG_GLOBAL_ATOMICS}.get(route, 0))
        h, _, st = g.render(lp)
        assert st.kernel_variant & capi.BF_VARIANT_EXACT_SUM and st.n_paths == RAGGED, route
        if route == "no_tail":
            assert st.n_bounces_tail == 0 and st.n_bounce_iters > 1
        if route == "default":
            assert st.n_bounces_tail > 0
            again = g.render(lp)[0]
            assert np.array_equal(bits(again), bits(h)), "the launch run twice"
        check_exact(h, exp, lp, f"route {route}")
        for other, ho in hists.items():
            assert np.array_equal(bits(h), bits(ho)), (route, other)
        hists[route] = h
        g.close()
    assert len(hists) == len(ROUTES)


def test_global_limbs_by_size(hiplib):
    """2560 bins: 2565 cells of 72 bytes do not fit the LDS; the five base channels go through the workgroup's table"""
    bins = 2560
    lp = _c4_launch(N, bins)
    g = capi.Scene(_c4())
    assert g.channels(lp) == 2565
    exp = Exact(cr.single_path_hists(_c4(), lp), N, 2565)
    h = _render_checked(g, lp)
    check_exact(h, exp, lp, "2560 bins")
    for extra in (capi.BF_FLAG_GLOBAL_ATOMICS, capi.BF_FLAG_MEGAKERNEL):
        assert np.array_equal(bits(g.render(summed(lp, extra))[0]), bits(h)), extra


def test_seeded_batch_equals_its_renders(hiplib):
    lp = _c4_launch()
    seeds = [3, 31, 32]
    g = capi.Scene(_c4())
    hb, rb, st = g.render_batch(summed(lp), 3, seeds=seeds, records=True)
    assert hb.shape == (3, 5 + BINS) and st.kernel_variant & capi.BF_VARIANT_EXACT_SUM
    hg, _, _ = g.render_batch(summed(lp, capi.BF_FLAG_GLOBAL_ATOMICS), 3, seeds=seeds)      # the table [render][5]
    for k in range(3):
        h1, r1, _ = g.render(summed(lp, seed=seeds[k]), records=True)
        _same_records(rb[k], r1)
        assert np.array_equal(bits(hb[k]), bits(h1)) and np.array_equal(bits(hg[k]), bits(h1)), k
    check_exact(hb[0], _c4_exact(), lp, "batch render 0")


def _mesh_vertices(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()


def test_motion_and_deform_batches_equal_pose_and_render(hiplib):
    sd = _c4()
    lp = _c4_launch()
    g, g2 = capi.Scene(sd), capi.Scene(sd)
    xf = np.tile(motion.rigid(), (3, len(sd.shapes), 1, 1)).astype(np.float32)
    xf[1, 4] = motion.rigid(t=(0.5, -1.75, 0.0))
    xf[2, 4] = motion.rigid(t=(1.0, -3.5, 0.0))
    hb, _, st = g.render_motion_batch(summed(lp), xf)
    assert hb.shape == (3, 5 + BINS) and st.kernel_variant & capi.BF_VARIANT_EXACT_SUM
    for k in range(3):
        g2.transform_meshes(xf[k])
        assert np.array_equal(bits(hb[k]), bits(g2.render(summed(lp))[0])), f"motion batch render {k}"
    assert not np.array_equal(bits(hb[0]), bits(hb[2]))
    g2.transform_meshes(xf[0])
    v = _mesh_vertices(sd, 4)
    c = 0.5 * (v.min(0) + v.max(0))
    pos = np.stack([v, ((v - c) * np.array([1.0, 1.0, 1.5], np.float32) + c + np.array([0.0, -1.0, 0.0], np.float32))]).astype(np.float32)
    hd, _, st = g.render_deform_batch(summed(lp), {4: pos})
    assert hd.shape == (2, 5 + BINS) and st.kernel_variant & capi.BF_VARIANT_EXACT_SUM
    for k in range(2):
        g2.update_vertices(4, pos[k])
        assert np.array_equal(bits(hd[k]), bits(g2.render(summed(lp))[0])), f"deform batch frame {k}"
    assert np.array_equal(bits(hd[0]), bits(hb[0])) and not np.array_equal(bits(hd[0]), bits(hd[1]))


def test_accumulates_into_the_callers_histogram(hiplib):
    """hist_dev comes back as fl(old + sum), one rounding; a cell without addends keeps its value, -0.0 included"""
    import torch
    lp = _c4_launch()
    exp = _c4_exact()
    n = 5 + BINS
    old = (np.random.default_rng(1).standard_normal(n) * 100.0).astype(np.float32)
    empty = np.flatnonzero(exp.N == 0)
    assert empty.size
    old[empty[0]] = -0.0
    buf = torch.from_numpy(old.copy()).cuda()
    g = capi.Scene(_c4())
    st = g.render_device(summed(lp), buf.data_ptr(), want_stats=True)
    assert st.kernel_variant & capi.BF_VARIANT_EXACT_SUM
    got = buf.cpu().numpy()
    live = np.flatnonzero(exp.N > 0).astype(np.uint32)
    want = old.copy()
    want[live] = capi.exact_sum(np.concatenate([exp.cells, live]), np.concatenate([exp.vals, old[live]]), n)[live]
    assert np.array_equal(bits(got), bits(want))
    # and once more on top: the handle's limbs were zeroed, the buffer's values are the new old ones
    g.render_device(summed(lp), buf.data_ptr())
    want2 = want.copy()
    want2[live] = capi.exact_sum(np.concatenate([exp.cells, live]), np.concatenate([exp.vals, want[live]]), n)[live]
    assert np.array_equal(bits(buf.cpu().numpy()), bits(want2))


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. behaviour
# ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hiplib):
    import torch
    sd = _c4()
    lp = _c4_launch()
    g = capi.Scene(sd)
    INVALID, UNSUPPORTED = capi.BF_ERR_INVALID, capi.BF_ERR_UNSUPPORTED
    g.set_classes([0, 1, 2, 3, 4], 6, 5)
    g.set_aovs(["depth"])
    combos = ((capi.BF_FLAG_FAST, "BF_FLAG_FAST"), (capi.BF_FLAG_MOMENT, "BF_FLAG_MOMENT"), (capi.BF_FLAG_CLASSES, "BF_FLAG_CLASSES"),
              (capi.BF_FLAG_AOV, "BF_FLAG_AOV"))
    xf = np.tile(motion.rigid(), (2, len(sd.shapes), 1, 1)).astype(np.float32)
    pos = np.stack([_mesh_vertices(sd, 4)] * 2)
    for extra, name in combos:
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM with {name}"):
            g.render(summed(lp, extra))
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM with {name}"):
            g.render_batch(summed(lp, extra), 2)
        # the motion / deform batch entries refuse before they prepare anything
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM with {name}"):
            g.render_motion_batch(summed(lp, extra), xf)
        with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM with {name}"):
            g.render_deform_batch(summed(lp, extra), {4: pos})
    g.clear_classes()
    # the limbs' headroom
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM.*2\^31"):
        g.render(summed(lp, n_paths=1 << 31))
    # shards
    buf = torch.zeros(5 + BINS, dtype=torch.float32, device="cuda")
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_EXACT_SUM"):
        capi.render_sharded([g], summed(lp))
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_EXACT_SUM"):
        capi.render_sharded_device([g], summed(lp), [buf.data_ptr()])
    # the converge entries force BF_FLAG_MOMENT
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM"):
        g.render_converge(summed(lp), 0.1, max_rounds=2)
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_EXACT_SUM"):
        g.render_converge_device(summed(lp), buf.data_ptr(), 0.1, max_rounds=2)
    # a rolling render: refused, and the open sequence stays intact
    seq = _Sequence(g, lp, [5, 6])
    seq.issue([0])
    with pytest.raises(capi.BeifongError, match=rf"status {UNSUPPORTED}\).*BF_FLAG_EXACT_SUM with BF_FLAG_ROLLING"):
        g.render_device(summed(lp, capi.BF_FLAG_ROLLING), buf.data_ptr())
    seq.issue([1])
    g.flush()
    h, recs = seq.results()
    assert float(buf.abs().sum()) == 0.0
    osc = OracleScene(sd)
    for k, seed in enumerate([5, 6]):
        _, ro, _, add = osc.render(copy_launch(lp, seed=seed), records=True, threads=8, addends=True)
        _same_records(recs[k], ro)
        assert_fp32_sum(h[k], add.ref, add.S, add.N, f"rolling render {k} around the refusal", counts=cr.count_channels(lp))
    # the handle is usable afterwards, with and without the flag
    check_exact(g.render(summed(lp))[0], _c4_exact(), lp, "after the refusals")
    h0, _, s0 = g.render(lp)
    assert not s0.kernel_variant & capi.BF_VARIANT_EXACT_SUM
    add = osc.render(lp, threads=8, addends=True)[3]
    assert_fp32_sum(h0, add.ref, add.S, add.N, "plain render after the refusals", counts=cr.count_channels(lp))
