"""Motion batches (bf_render_motion_batch): every render of one batch moves the meshes by its own rigid transforms.
Render k is held, path for path, to bf_scene_transform_meshes(xf[k]) plus a stand-alone render on a second handle, and once to
the oracle on a scene rebuilt from the moved vertices; the handle itself, its pose and its clones are left as they were."""
import ctypes as C

import numpy as np
import pytest

from beifong_amd import capi, motion
from tests.hist_bound import assert_fp32_sum, assert_two_fp32_sums, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _launch_like, _same_records
from tests.test_gpu_motion import _identity, _meshes, _multi_mesh, _poses, _receive_iq, _two_plates

pytestmark = pytest.mark.gpu


def _batch_poses(sd, n):
    """n transform tables: the identity, then _poses' variants (every mesh its own turn and shift)."""
    return np.stack([_identity(sd)] + [_poses(sd, v) for v in range(n - 1)]).astype(np.float32)


def _flags(lp, flags):
    return _launch_like(lp, lp.seed, flags=lp.flags | flags)


def _assert_like_transform_then_render(sd, lp, xf, seeds, hb, rb, st):
    """render k of a batch == transform_meshes(xf[k]) + a stand-alone render with seed seeds[k], on another handle"""
    ref = capi.Scene(sd)
    n = int(lp.n_paths)
    for k in range(xf.shape[0]):
        ref.transform_meshes(xf[k])
        hs, rs, ss = ref.render(_launch_like(lp, lp.seed if seeds is None else int(seeds[k]), flags=lp.flags), records=True)
        _same_records(rb[k], rs)
        amax = float(np.abs(rs["L"]).max()) if n else 1.0
        assert np.allclose(hb[k], hs, rtol=2e-5, atol=n * 2.0 ** -24 * max(amax, 1.0) * 4), k
    assert st.n_paths == xf.shape[0] * n and st.n_guard == 0
    ref.close()


@pytest.mark.parametrize("seeded", [False, True], ids=["common_seed", "own_seeds"])
@pytest.mark.parametrize("case", ["range", "range_normals", "receive_iq"])
def test_batch_equals_transform_then_render(hiplib, case, seeded):
    sd, lp = _receive_iq() if case == "receive_iq" else _multi_mesh(case == "range_normals")
    xf = _batch_poses(sd, 4)
    seeds = np.array([11, 12, 13, 14], np.uint64) if seeded else None
    g = capi.Scene(sd)
    hb, rb, st = g.render_motion_batch(lp, xf, seeds=seeds, records=True)
    assert not np.array_equal(rb[0]["L"], rb[1]["L"])           # the motion shows
    _assert_like_transform_then_render(sd, lp, xf, seeds, hb, rb, st)


def test_batch_against_the_oracle(hiplib):
    """One render of a batch against the oracle on a scene rebuilt from motion.apply_rigid vertices: records and every
    histogram cell within its fp32 summation bound."""
    sd, lp = _multi_mesh(True)
    xf = _batch_poses(sd, 3)
    hb, rb, _ = capi.Scene(sd).render_motion_batch(lp, xf, records=True)
    k = 2
    fresh = motion.moved_description(sd, xf[k])
    _, ro, _, add = OracleScene(fresh).render(lp, records=True, threads=8, addends=True)
    _same_records(rb[k], ro)
    assert_fp32_sum(hb[k], add.ref, add.S, add.N, "motion batch render 2", counts=count_channels(lp, fresh))


def test_deep_tail(hiplib):
    """2^18 paths per render: the tail kernel finishes long paths of several renders side by side."""
    sd, _ = _multi_mesh(False)
    lp = capi.make_launch(capi.BF_MODE_RANGE, 1 << 18, seed=5, bins=1024, bin_width=0.03)
    xf = _batch_poses(sd, 3)
    hb, rb, st = capi.Scene(sd).render_motion_batch(lp, xf, seeds=[1, 2, 3], records=True)
    assert st.n_rays_tail > 0
    _assert_like_transform_then_render(sd, lp, xf, [1, 2, 3], hb, rb, st)


@pytest.mark.parametrize("mode", ["fast", "megakernel", "no_wide", "quant"])
def test_modes_and_tree_variants(hiplib, monkeypatch, mode):
    if mode == "no_wide":
        monkeypatch.setenv("BF_NO_WIDE_BVH", "1")
    if mode == "quant":
        monkeypatch.setenv("BF_QUANT_BVH", "1")
    flags = {"fast": capi.BF_FLAG_FAST, "megakernel": capi.BF_FLAG_MEGAKERNEL}.get(mode, 0)
    for sd, lp in (_multi_mesh(True), _receive_iq()):
        lp = _flags(lp, flags)
        xf = _batch_poses(sd, 3)
        g = capi.Scene(sd)
        if mode == "quant":
            assert g.info().trace_node_bytes == 64
        hb, rb, st = g.render_motion_batch(lp, xf, seeds=[7, 8, 9], records=True)
        _assert_like_transform_then_render(sd, lp, xf, [7, 8, 9], hb, rb, st)


def test_handle_and_clones_are_untouched(hiplib):
    """The handle keeps its own pose (a transform it holds included), its clones theirs, and a batch on a clone leaves the
    source alone; a second batch of other poses reuses the arena."""
    sd, lp = _multi_mesh(True)
    a = _poses(sd, 1)
    g = capi.Scene(sd)
    g.transform_meshes(a)
    c = g.clone()
    u = capi.Scene(sd)                 # a handle that never moved
    cu = u.clone()
    _, rg0, _ = g.render(lp, records=True)
    _, rc0, _ = c.render(lp, records=True)
    _, ru0, _ = u.render(lp, records=True)
    xf = _batch_poses(sd, 3)
    hb, rb, st = g.render_motion_batch(lp, xf, records=True)
    _assert_like_transform_then_render(sd, lp, xf, None, hb, rb, st)    # absolute from the geometry as created, not from `a`
    _, rg1, _ = g.render(lp, records=True)
    _same_records(rg1, rg0)
    _, rc1, _ = c.render(lp, records=True)
    _same_records(rc1, rc0)
    u.render_motion_batch(lp, xf[::-1].copy())
    _, ru1, _ = u.render(lp, records=True)
    _same_records(ru1, ru0)
    _, rcu, _ = cu.render(lp, records=True)
    _same_records(rcu, ru0)
    c.render_motion_batch(lp, xf)
    _, rg2, _ = g.render(lp, records=True)
    _same_records(rg2, rg0)
    xf2 = np.stack([_poses(sd, 2), _poses(sd, 0)])
    hb2, rb2, st2 = g.render_motion_batch(lp, xf2, records=True)
    _assert_like_transform_then_render(sd, lp, xf2, None, hb2, rb2, st2)
    # the handle's transform still works on its own geometry after batches
    g.transform_meshes(xf2[0])
    _, rg3, _ = g.render(lp, records=True)
    _same_records(rg3, rb2[0])


def test_small_arena_renders_in_chunks(hiplib, monkeypatch):
    sd, lp = _multi_mesh(True)
    xf = _batch_poses(sd, 5)
    seeds = [3, 1, 4, 1, 5]
    hb, rb, st = capi.Scene(sd).render_motion_batch(lp, xf, seeds=seeds, records=True)
    monkeypatch.setenv("BF_MOTION_BATCH_MB", "1")          # below one version of this scene: one render per chunk
    g = capi.Scene(sd)
    hc, rc, sc = g.render_motion_batch(lp, xf, seeds=seeds, records=True)
    for k in range(len(seeds)):
        _same_records(rc[k], rb[k])
    assert sc.n_paths == st.n_paths == len(seeds) * lp.n_paths and sc.n_guard == 0
    assert sc.n_bounce_iters > st.n_bounce_iters                  # several launch sequences
    amax = float(np.abs(rb["L"]).max())
    assert np.allclose(hc, hb, rtol=2e-5, atol=lp.n_paths * 2.0 ** -24 * max(amax, 1.0) * 4)
    monkeypatch.setenv("BF_MOTION_BATCH_MB", "24")         # a few versions per chunk
    hd, rd, _ = g.render_motion_batch(lp, xf, seeds=seeds, records=True)
    for k in range(len(seeds)):
        _same_records(rd[k], rb[k])


def _status(g, lp, xf, n_renders=None, n_shapes=None, seeds=None):
    xf = np.ascontiguousarray(xf, np.float32)
    n_renders = xf.shape[0] if n_renders is None else n_renders
    n_shapes = xf.shape[1] if n_shapes is None else n_shapes
    ch = g.channels(lp)
    hist = np.zeros(max(1, n_renders) * ch, np.float32)
    return g.lib.bf_render_motion_batch(g.handle, C.byref(lp), n_renders, None, n_shapes, xf.ctypes.data_as(C.c_void_p),
                                        hist.ctypes.data_as(C.c_void_p), None, None)


def test_refused_inputs_leave_the_scene_intact(hiplib):
    sd, lp = _multi_mesh(True)
    g = capi.Scene(sd)
    g.transform_meshes(_poses(sd, 1))
    _, r0, _ = g.render(lp, records=True)
    good = _batch_poses(sd, 3)
    k = _meshes(sd)[1]
    rect = next(i for i, s in enumerate(sd.shapes) if s.type != capi.BF_SHAPE_MESH and s.emitter < 0)
    bad = []
    for edit in ("scale", "shear", "mirror", "nan", "rect"):
        x = good.copy()
        if edit == "scale":
            x[2, k, :, :3] *= np.float32(1.01)
        elif edit == "shear":
            x[1, k, 0, 1] += np.float32(0.05)
        elif edit == "mirror":
            x[2, k, :, 0] *= -1
        elif edit == "nan":
            x[1, k, 1, 3] = np.nan
        else:
            x[2, rect] = motion.rigid(t=(0.0, 0.0, 0.1))
        bad.append(x)
    for x in bad:
        assert _status(g, lp, x) == capi.BF_ERR_INVALID
    msg = hiplib.bf_last_error().decode()
    assert "render 2" in msg and "shape %d" % rect in msg, msg
    assert _status(g, lp, good, n_shapes=len(sd.shapes) - 1) == capi.BF_ERR_INVALID
    assert _status(g, lp, good, n_renders=0) == capi.BF_ERR_INVALID
    assert _status(g, _flags(lp, capi.BF_FLAG_ROLLING), good) == capi.BF_ERR_INVALID
    _, r1, _ = g.render(lp, records=True)
    _same_records(r1, r0)
    # a moved mesh that carries an emitter: unsupported, render and shape named
    sd2, lp2 = _multi_mesh(False)
    m0 = _meshes(sd2)[0]
    sd2.shapes[m0].emitter = 0
    sd2.finalize()
    g2 = capi.Scene(sd2)
    _, q0, _ = g2.render(lp2, records=True)
    x2 = _batch_poses(sd2, 2)
    assert _status(g2, lp2, x2) == capi.BF_ERR_UNSUPPORTED
    msg = hiplib.bf_last_error().decode()
    assert "render 1" in msg and "shape %d" % m0 in msg, msg
    _, q1, _ = g2.render(lp2, records=True)
    _same_records(q1, q0)


def test_multi_pixel_film_is_refused(hiplib):
    from beifong_amd import scenes
    sd, lp = scenes.film_half_lit(film=(4, 2), spp=16)
    g = capi.Scene(sd)
    xf = np.stack([_identity(sd)] * 2).astype(np.float32)
    assert _status(g, lp, xf) == capi.BF_ERR_INVALID
    assert "multi-pixel" in hiplib.bf_last_error().decode()


def test_open_rolling_sequence_is_flushed(hiplib):
    """A motion batch finishes the handle's open rolling sequence first: every rolling render is complete (W = its valid
    paths) and path for path a stand-alone render; the batch's own histograms are complete too."""
    pytest.importorskip("torch")
    sd, lp = _multi_mesh(False)
    g = capi.Scene(sd)
    seeds = [31, 32, 33]
    seq = _Sequence(g, lp, seeds)
    seq.issue()
    xf = _batch_poses(sd, 2)
    hb, rb, st = g.render_motion_batch(lp, xf, records=True)
    h, recs = seq.results()
    for k, seed in enumerate(seeds):
        hs, rs, ss = capi.Scene(sd).render(_launch_like(lp, seed), records=True)
        _same_records(recs[k], rs)
        assert h[k][4] == hs[4] == lp.n_paths - ss.n_invalid
    _assert_like_transform_then_render(sd, lp, xf, None, hb, rb, st)
    ref = capi.Scene(sd)
    for k in range(2):
        ref.transform_meshes(xf[k])
        hs, _, ss = ref.render(lp)
        assert hb[k][4] == hs[4] == lp.n_paths - ss.n_invalid


def test_motion_sweep_batched_against_per_pulse(hiplib):
    """render_motion_sweep's batches against its per-pulse reference: every cell within the fp32 summation bound of the
    pulse's addends (from the oracle for a few pulses, and the W count exact), Doppler lines where the speeds put them."""
    pytest.importorskip("torch")
    from beifong_amd import sweep
    lam, n_pulses = 0.1, 64
    dx = (-0.004, -0.0125)
    sd, lp, plates = _two_plates(*dx)
    xf = np.tile(_identity(sd)[None], (n_pulses, 1, 1, 1)).astype(np.float32)
    for i, k in enumerate(plates):
        xf[:, k, 0, 3] = dx[i] * np.arange(n_pulses)
    cb = sweep.render_motion_sweep(sd, lp, xf, n_streams=2)
    cp = sweep.render_motion_sweep(sd, lp, xf, n_streams=2, per_pulse=True)
    assert cb.shape == cp.shape == (n_pulses, 1, 3)
    assert np.array_equal(cb[:, :, 2], cp[:, :, 2]) and np.all(cb[:, 0, 2] == lp.n_paths)
    for k in (0, 17, 63):
        _, _, _, add = OracleScene(motion.moved_description(sd, xf[k])).render(lp, records=False, threads=8, addends=True)
        assert_two_fp32_sums(cb[k].reshape(-1), cp[k].reshape(-1), add.S, add.N, f"motion sweep pulse {k}")
    scale = np.abs(cp[:, :, :2]).max()
    assert np.allclose(cb, cp, rtol=1e-4, atol=1e-6 * scale)
    rd = np.abs(sweep.range_doppler(cb)[:, 0])
    top = {int(x) for x in np.argsort(rd)[::-1][:8]}
    floor = np.median(rd)
    for i in range(2):
        expect = int(round(2 * abs(dx[i]) / lam * n_pulses)) % n_pulses
        assert expect in top or (expect + 1) % n_pulses in top, (i, expect, sorted(top))
        assert max(rd[expect], rd[(expect + 1) % n_pulses]) > 10 * floor
