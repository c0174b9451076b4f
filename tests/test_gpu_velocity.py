"""Range rate from per-vertex velocities (Scene.set_velocity_mode under Scene.set_range_rate_classes): a mesh in
BF_VELOCITY_VERTEX or BF_VELOCITY_DIFFERENCE adds the velocity interpolated at the hit to its shape's twist.  Expected cells come
from the unchanged oracle through tests/velocity_ref.py (every path's composed primary ray, the shape, face and barycentrics it
meets first -> capi.interpolate_velocity of capi.corner_velocities or of the explicit field -> capi.range_rate_classes ->
class_ref.per_class: every path rendered alone).  Every block of every device histogram is held to its per-cell fp32 summation
bound, the count channels exact per class, the per-path records bit-equal to the oracle's.  The scene is tests/velocity_ref.py's:
front end, ground, bus and the three-bone bar, 8192 paths, bins [-1, 0) m/s in 8, every twist zero, dt = 1/64 s."""
import functools

import numpy as np
import pytest

from beifong_amd import capi, motion
from tests import class_ref as cr
from tests import range_rate_ref as rr
from tests import velocity_ref as vr
from tests.moment_ref import copy_launch
from tests.rolling_helpers import _same_records

pytestmark = pytest.mark.gpu
f32 = np.float32
TWIST, VERTEX, DIFF = capi.BF_VELOCITY_TWIST, capi.BF_VELOCITY_VERTEX, capi.BF_VELOCITY_DIFFERENCE
CLS = capi.BF_FLAG_CLASSES
ANGLES = [(20.0, -30.0), (21.0, -32.0), (22.0, -34.0), (23.0, -36.0)]      # four consecutive instants of the bar
N_CLASSES = vr.N_BINS + 2


def _S():
    return vr.scene()[2]


def _bones(angles=ANGLES):
    return np.ascontiguousarray(np.stack([vr.bend(_S(), list(a)) for a in angles]), f32)


def _P(k, dq=False):
    return vr._vertices(ANGLES[k], dq)


def _pair(k, n=len(ANGLES)):
    """the two versions render k of an n-render batch differences: (k, k + 1), the last render the pair before it"""
    return (k, k + 1) if k < n - 1 else (n - 2, n - 1)


_SINGLES, _EXPECTED = {}, {}


def _exp(P, V, sd=None, lp=None, k=None, bins=None, twists=None, twin=None, others=None):
    """(Expected, oracle records) of the scene with shape k (the bar) standing at the world-space vertices P and moving with the
    per-vertex field V (others: {shape: vertices} of further meshes that stand elsewhere, in BF_VELOCITY_TWIST); computed once per
    (P, V, launch) and shared"""
    sd0, lp0, S = vr.scene()
    sd, lp, k = sd if sd is not None else sd0, lp if lp is not None else lp0, S.k if k is None else k
    P, V = np.ascontiguousarray(P, f32), np.ascontiguousarray(V, f32)
    tw = vr.still(sd) if twists is None else np.asarray(twists, f32)
    others = {int(j): np.ascontiguousarray(q, f32) for j, q in (others or {}).items()}
    key = (id(sd), int(lp.n_paths), int(lp.mode), int(lp.seed), P.tobytes() + b"".join(q.tobytes() for _, q in sorted(others.items())), V.tobytes(),
           tw.tobytes(), None if bins is None else (bins.r0, bins.r1, bins.n_bins))
    if key not in _EXPECTED:
        on = motion.deformed_description(sd, {**others, k: P})
        skey = key[:5]
        if skey not in _SINGLES:
            _SINGLES[skey] = cr.single_path_hists(on, lp)
        e, rec, _ = vr.expected(sd, lp, bins if bins is not None else vr.table(), tw, {k: V}, twin=twin, singles=_SINGLES[skey], trace_sd=on)
        _EXPECTED[key] = (e, rec)
    return _EXPECTED[key]


def _cv(a, b, dt=vr.DT):
    return capi.corner_velocities(a, b, dt)


def _scene(mode=DIFF, dt=vr.DT, table_first=True, skin=True):
    sd, lp, S = vr.scene()
    g = capi.Scene(sd)
    if skin:
        g.set_skin(S.k, S.n_bones, S.rest, S.index, S.weight)
    if table_first:
        assert g.set_range_rate_classes(vr.table(), vr.still(sd)) == N_CLASSES
    g.set_velocity_mode(S.k, mode, dt)
    if not table_first:
        assert g.set_range_rate_classes(vr.table(), vr.still(sd)) == N_CLASSES
    return g


def _check(h, rec, exp_rec, what, populated=3):
    exp, rec_o = exp_rec
    if rec is not None:
        _same_records(rec, rec_o)
    exp.check(h, what)
    assert (exp.population()[:vr.N_BINS] > 0).sum() >= populated, (what, exp.population())      # nothing is vacuous: the field shows
    return exp


def _lp():
    return cr.classed(vr.scene()[1])


# ---- BF_VELOCITY_DIFFERENCE in a batch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["whole", "chunked", "dq"])
def test_skin_batch(hiplib, monkeypatch, case):
    """4 renders of 4 consecutive poses: render k carries the forward difference to pose k + 1, the last render the field of the
    one before it at its own pose; cut to one render per chunk, every chunk needs the first version of the next (the last: the one
    before it)"""
    dq = case == "dq"
    g = _scene()
    if dq:
        g.set_skin_mode(_S().k, capi.BF_SKIN_DUAL_QUATERNION)
    if case == "chunked":
        monkeypatch.setenv("BF_MOTION_BATCH_MB", "0")        # below one version: one render per chunk
    hb, rb, st = g.render_skin_batch(_lp(), {_S().k: _bones()}, records=True)
    monkeypatch.delenv("BF_MOTION_BATCH_MB", raising=False)
    assert hb.shape == (4, N_CLASSES * (1024 + 5)) and st.kernel_variant & capi.BF_VARIANT_CLASS
    g.sync()
    seen = []
    for k in range(4):
        a, b = _pair(k)
        e = _check(hb[k], rb[k], _exp(_P(k, dq), _cv(_P(a, dq), _P(b, dq))), f"skin batch {case}, render {k}", populated=8)
        seen.append(e.cls)
    if not dq:
        bar = vr.bar_expected(ANGLES[0], ANGLES[0], ANGLES[1])[0]
        assert np.array_equal(bar.cls, seen[0]) and bar.population()[:vr.N_BINS].tolist() == vr.BAR_POPULATION[0]
    assert not np.array_equal(seen[2], seen[3])              # the same field at another pose
    # the handle's own field is untouched by a batch, as its pose is: zero, at the rest pose
    h, rec, _ = g.render(_lp(), records=True)
    e0, r0 = _exp(_S().rest, np.zeros_like(_S().rest))
    _same_records(rec, r0)
    e0.check(h, "the handle after the batch")
    assert e0.population()[:vr.N_BINS].sum() == 0


def _bar_xf(n, k, step):
    sd, _, S = vr.scene()
    xf = np.tile(motion.rigid(), (n, len(sd.shapes), 1, 1)).astype(f32)
    for i in range(n):
        xf[i, k] = motion.about(motion.rotation([0.1, 0.3, 1.0], step * i), S.joints[0], (-0.004 * i, 0.002 * i, 0.0))
    return xf


def test_skin_batch_with_transforms(hiplib):
    """per-render transforms on top of the poses: the differenced positions are the transformed ones"""
    S = _S()
    xf = _bar_xf(4, S.k, 0.4)
    g = _scene()
    hb, rb, _ = g.render_skin_batch(_lp(), {S.k: _bones()}, transforms=xf, records=True)
    P = [motion.apply_rigid(_P(k), None, xf[k, S.k])[0] for k in range(4)]
    assert not np.array_equal(P[1], _P(1))
    for k in range(4):
        a, b = _pair(k)
        _check(hb[k], rb[k], _exp(P[k], _cv(P[a], P[b])), f"skin batch with transforms, render {k}", populated=6)


def _targets():
    S = _S()
    x = S.rest.astype(np.float64)
    c = x.mean(0)
    d0 = 0.02 * (x - c) * np.sin(3.0 * x[:, :1])             # a breathing mode
    d1 = np.stack([0.01 * np.cos(2.0 * x[:, 1]), 0.015 * np.sin(x[:, 0]), np.zeros(len(x))], -1)
    return np.ascontiguousarray(np.stack([d0, d1]), f32)


def test_morph_batch(hiplib):
    S = _S()
    dp = _targets()
    w = np.array([[0.0, 0.0], [0.3, -0.2], [0.55, -0.45], [0.7, -0.8]], f32)
    g = _scene(skin=False)
    g.set_morph(S.k, 2, S.rest, dp)
    hb, rb, _ = g.render_morph_batch(_lp(), {S.k: w}, records=True)
    P = [motion.apply_morph(S.rest, None, dp, None, w[k])[0] for k in range(4)]
    for k in range(4):
        a, b = _pair(k)
        _check(hb[k], rb[k], _exp(P[k], _cv(P[a], P[b])), f"morph batch, render {k}", populated=2)


def test_deform_batch(hiplib):
    S = _S()
    P = [np.ascontiguousarray(S.rest + f32(k) * _targets()[0] - f32(0.003 * k) * np.array([1.0, 0.5, 0.0], f32), f32) for k in range(3)]
    g = _scene(skin=False)
    hb, rb, _ = g.render_deform_batch(_lp(), {S.k: np.stack(P)}, records=True)
    for k in range(3):
        a, b = _pair(k, 3)
        _check(hb[k], rb[k], _exp(P[k], _cv(P[a], P[b])), f"deform batch, render {k}", populated=2)


def test_motion_batch(hiplib):
    """a rigid motion of the bar, differenced: what a twist would state, from the rows"""
    S = _S()
    xf = _bar_xf(3, S.k, 0.5)
    g = _scene(skin=False)
    hb, rb, _ = g.render_motion_batch(_lp(), xf, records=True)
    P = [motion.apply_rigid(S.rest, None, xf[k, S.k])[0] for k in range(3)]
    for k in range(3):
        a, b = _pair(k, 3)
        _check(hb[k], rb[k], _exp(P[k], _cv(P[a], P[b])), f"motion batch, render {k}")


# ---- BF_VELOCITY_DIFFERENCE on a handle ----------------------------------------------------------------------------------------------
def test_handle_moves(hiplib):
    """zero before the first move; every move differences the rendered rows before and after it: two poses, a transform between
    two poses, and a pose under that transform"""
    sd, _, S = vr.scene()
    g = _scene()
    assert g.get_velocity_mode(S.k) == (DIFF, vr.DT) and g.get_velocity_mode(S.k - 1) == (TWIST, 0.0)
    zero = np.zeros_like(S.rest)
    h, rec, _ = g.render(_lp(), records=True)
    e = _check(h, rec, _exp(S.rest, zero), "before the first move", populated=0)
    assert e.population()[:vr.N_BINS].sum() == 0
    bones = _bones()
    g.pose_skin(S.k, bones[0])
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, _exp(_P(0), _cv(S.rest, _P(0))), "first pose: from the rest pose")
    g.pose_skin(S.k, bones[1])
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, _exp(_P(1), _cv(_P(0), _P(1))), "second pose: the backward difference", populated=8)
    xf = _bar_xf(2, S.k, 0.6)[1]
    g.transform_meshes(xf)
    Q1 = motion.apply_rigid(_P(1), None, xf[S.k])[0]
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, _exp(Q1, _cv(_P(1), Q1)), "a transform between two poses")
    g.pose_skin(S.k, bones[2])
    Q2 = motion.apply_rigid(_P(2), None, xf[S.k])[0]
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, _exp(Q2, _cv(Q1, Q2)), "a pose under the transform")
    # a translation replaces the transform, for every mesh: the bus moves too, in BF_VELOCITY_TWIST, and carries no field
    off = np.array([0.01, -0.005, 0.0], f32)
    g.translate_meshes(off)
    Q3 = (_P(2) + off).astype(f32)
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, _exp(Q3, _cv(Q2, Q3), others={S.k - 1: (vr._verts(sd, S.k - 1) + off).astype(f32)}), "a translation in place of the transform",
           populated=0)
    g.sync()


def test_skin_sweep_with_velocities(hiplib):
    """render_skin_sweep(..., classes=, velocities=) on one stream: per pulse the backward differences of the per-pulse calls, in
    batches the forward differences of the skin batch"""
    from beifong_amd import sweep
    sd, lp, S = vr.scene()
    skins, bones = {S.k: (S.index, S.weight)}, {S.k: _bones()}
    classes = (vr.table(), vr.still(sd))
    cube = sweep.render_skin_sweep(sd, lp, skins, bones, n_streams=1, per_pulse=True, classes=classes, velocities={S.k: vr.DT})
    assert cube.shape == (4, N_CLASSES, (1024 + 5) // 3, 3)
    g = _scene()
    for k in range(4):
        g.pose_skin(S.k, bones[S.k][k])
        h, rec, _ = g.render(_lp(), records=True)
        e = _check(h, rec, _exp(_P(k), _cv(S.rest if k == 0 else _P(k - 1), _P(k))), f"per-pulse call {k}")
        e.check(cube[k], f"sweep pulse {k}")
        e.check_two(cube[k], h, f"sweep pulse {k} against the per-pulse call")
    batched = sweep.render_skin_sweep(sd, lp, skins, bones, n_streams=1, classes=classes, velocities={S.k: vr.DT})
    for k in range(4):
        a, b = _pair(k)
        _exp(_P(k), _cv(_P(a), _P(b)))[0].check(batched[k], f"batched sweep pulse {k}")


def _exp2(bar_P, bar_V, bus_P, bus_V):
    """_exp with a field on the bus too: (Expected, oracle records)"""
    sd, lp, S = vr.scene()
    on = motion.deformed_description(sd, {S.k: np.ascontiguousarray(bar_P, f32), S.k - 1: np.ascontiguousarray(bus_P, f32)})
    e, rec, _ = vr.expected(sd, lp, vr.table(), vr.still(sd), {S.k: bar_V, S.k - 1: bus_V}, singles=cr.single_path_hists(on, lp), trace_sd=on)
    return e, rec


def _bus(k):
    """the bus at instant k: drifting towards the radar, 8 mm an instant (0.5 m/s over dt)"""
    sd, _, S = vr.scene()
    return (vr._verts(sd, S.k - 1) + f32(k) * np.array([-0.008, 0.001, 0.0], f32)).astype(f32)


def test_two_shapes_moved_in_turn(hiplib):
    """two meshes in BF_VELOCITY_DIFFERENCE on one handle: a call that moves one of them leaves the other's field as it is (its rows
    are rewritten with what they held: that is no move), on the handle and through a per-pulse sweep that moves both every pulse"""
    from beifong_amd import sweep
    sd, lp, S = vr.scene()
    bus = S.k - 1
    g = _scene()
    g.set_velocity_mode(bus, DIFF, vr.DT)
    g.pose_skin(S.k, _bones()[0])
    g.pose_skin(S.k, _bones()[1])
    g.update_vertices(bus, _bus(1))                          # the bar keeps the difference of its two poses
    h, rec, _ = g.render(_lp(), records=True)
    e = _check(h, rec, _exp2(_P(1), _cv(_P(0), _P(1)), _bus(1), _cv(_bus(0), _bus(1))), "bar posed twice, then the bus", populated=8)
    bar_alone = _exp(_P(1), _cv(_P(0), _P(1)), others={bus: _bus(1)})[0]
    assert not np.array_equal(e.cls, bar_alone.cls)          # the bus's own field shows too
    g.pose_skin(S.k, _bones()[2])                            # ... and the bus keeps its field when the bar moves on
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, _exp2(_P(2), _cv(_P(1), _P(2)), _bus(1), _cv(_bus(0), _bus(1))), "then the bar again", populated=8)
    g.sync()
    # the per-pulse deform sweep updates both shapes every pulse, one after the other (two streams asked for: one is used)
    pos = {bus: np.stack([_bus(k) for k in range(3)]), S.k: np.stack([_P(k) for k in range(3)])}
    cube = sweep.render_deform_sweep(sd, lp, pos, n_streams=2, per_pulse=True, classes=(vr.table(), vr.still(sd)), velocities={bus: vr.DT, S.k: vr.DT})
    for k in (1, 2):
        _exp2(_P(k), _cv(_P(k - 1), _P(k)), _bus(k), _cv(_bus(k - 1), _bus(k)))[0].check(cube[k], f"per-pulse sweep, pulse {k}")
    batched = sweep.render_deform_sweep(sd, lp, pos, n_streams=2, classes=(vr.table(), vr.still(sd)), velocities={bus: vr.DT, S.k: vr.DT})
    for k in range(3):
        a, b = _pair(k, 3)
        _exp2(_P(k), _cv(_P(a), _P(b)), _bus(k), _cv(_bus(a), _bus(b)))[0].check(batched[k], f"batched sweep, pulse {k}")


# ---- BF_VELOCITY_VERTEX --------------------------------------------------------------------------------------------------------------
def _spin(P, omega=(0.0, 0.0, 1.5), pivot=None):
    """omega x (P - pivot) per vertex, in float32"""
    pivot = np.asarray(_S().joints[1] if pivot is None else pivot, f32)
    return np.ascontiguousarray(np.cross(np.asarray(omega, f32), (np.asarray(P, f32) - pivot).astype(f32)), f32)


def test_explicit_field(hiplib):
    import torch
    sd, _, S = vr.scene()
    g = _scene(VERTEX)
    assert g.get_velocity_mode(S.k) == (VERTEX, 0.0)
    zero = np.zeros_like(S.rest)
    h, rec, _ = g.render(_lp(), records=True)
    assert _check(h, rec, _exp(S.rest, zero), "zero until a field is given", populated=0).population()[:vr.N_BINS].sum() == 0
    V = _spin(S.rest)
    g.set_vertex_velocities(S.k, V)
    h, rec, _ = g.render(_lp(), records=True)
    e = _check(h, rec, _exp(S.rest, V), "an omega x r field", populated=6)
    # the device form, another field
    V2 = _spin(S.rest, omega=(0.3, -0.2, -2.0))
    t = torch.from_numpy(V2).cuda()
    g.set_vertex_velocities(S.k, t.data_ptr(), device=True)
    g.sync()
    h, rec, _ = g.render(_lp(), records=True)
    e2 = _check(h, rec, _exp(S.rest, V2), "the device form")
    assert not np.array_equal(e.cls, e2.cls)
    # moves leave an explicit field alone; a batch shares it among its renders
    g.set_vertex_velocities(S.k, V)
    hb, rb, _ = g.render_skin_batch(_lp(), {S.k: _bones()[:2]}, records=True)
    for k in range(2):
        _check(hb[k], rb[k], _exp(_P(k), V), f"a batch that shares the field, render {k}", populated=6)
    g.pose_skin(S.k, _bones()[1])
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, _exp(_P(1), V), "after a pose", populated=6)
    # None: zeros again
    g.set_vertex_velocities(S.k, None)
    assert _check(g.render(_lp())[0], None, _exp(_P(1), zero), "the field cleared", populated=0).population()[:vr.N_BINS].sum() == 0


# ---- routes --------------------------------------------------------------------------------------------------------------------------
def _posed_twice(g):
    g.pose_skin(_S().k, _bones()[0])
    g.pose_skin(_S().k, _bones()[1])
    return _exp(_P(1), _cv(_P(0), _P(1)))


def test_global_atomics_and_one_kernel_variant(hiplib):
    g = _scene()
    want = _posed_twice(g)
    h = g.render(_lp())[0]
    for extra, route in ((capi.BF_FLAG_GLOBAL_ATOMICS, "global atomics"), (capi.BF_FLAG_MEGAKERNEL, "one-kernel variant")):
        hr, rec, st = g.render(cr.classed(vr.scene()[1], extra), records=True)
        assert st.kernel_variant & capi.BF_VARIANT_CLASS
        _check(hr, rec, want, route, populated=8).check_two(hr, h, f"{route} against the default route")


def test_regeneration_and_tail(hiplib, monkeypatch):
    """1024 slots for 4096 + 37 paths: a regenerated slot's class is its new path's, and the tail kernel reads the rows too"""
    sd, lp, S = vr.scene()
    lp = copy_launch(lp, n_paths=4096 + 37)
    with monkeypatch.context() as m:
        m.setenv("BF_WF_POOL", "1024")
        g = capi.Scene(sd)
    g.set_skin(S.k, S.n_bones, S.rest, S.index, S.weight)
    g.set_range_rate_classes(vr.table(), vr.still(sd))
    g.set_velocity_mode(S.k, DIFF, vr.DT)
    _posed_twice(g)
    h, rec, st = g.render(cr.classed(lp), records=True)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS and st.n_paths == 4096 + 37 and st.n_bounces_tail > 0
    _check(h, rec, _exp(_P(1), _cv(_P(0), _P(1)), lp=lp), "pool of 1024 slots", populated=8)


@functools.lru_cache(maxsize=None)
def _rx():
    return vr.receive_scene(4096)


@functools.lru_cache(maxsize=None)
def _rx_twin():
    return cr.fluxmeter_twin(lambda: vr.receive_scene(4096)[0])


@pytest.mark.parametrize("mode", [capi.BF_MODE_RECEIVE_RAW, capi.BF_MODE_RECEIVE_IQ], ids=["raw", "iq"])
def test_receive(hiplib, mode):
    """the bar in the bus's place before the receiver: two poses, the backward difference, through the receive kernels"""
    sd, lp, S = _rx()
    lp = copy_launch(lp, mode=mode)
    bins = capi.range_rate_bins((-2.0, 2.0), 8)
    g = capi.Scene(sd)
    g.set_skin(S.k, S.n_bones, S.rest, S.index, S.weight)
    g.set_range_rate_classes(bins, vr.still(sd))
    g.set_velocity_mode(S.k, DIFF, vr.DT)
    P = [motion.apply_skin(S.rest, None, S.index, S.weight, vr.bend(S, list(a)))[0] for a in ANGLES[:2]]
    for a in ANGLES[:2]:
        g.pose_skin(S.k, vr.bend(S, list(a)))
    h, rec, st = g.render(cr.classed(lp), records=True)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS
    _check(h, rec, _exp(P[1], _cv(P[0], P[1]), sd=sd, lp=lp, k=S.k, bins=bins, twin=_rx_twin()), f"receive mode {mode}", populated=4)


def test_film(hiplib):
    """the 8 x 6 film of the range-rate tests, its bus spinning by an explicit field on top of its twist"""
    sd, lp = cr.film_scene()
    k = len(sd.shapes) - 1
    b, tw = rr.table("film"), rr.twists(sd)
    P = vr._verts(sd, k)
    V = _spin(P, omega=(0.0, 0.0, -0.4), pivot=P.mean(0))
    g = capi.Scene(sd)
    assert g.set_range_rate_classes(b, tw) == 8
    g.set_velocity_mode(k, VERTEX)
    g.set_vertex_velocities(k, V)
    h, rec, st = g.render(cr.classed(lp), records=True)
    assert st.kernel_variant & capi.BF_VARIANT_CLASS
    e = _check(h, rec, _exp(P, V, sd=sd, lp=lp, k=k, bins=b, twists=tw), "8 x 6 film", populated=4)
    assert not np.array_equal(e.cls, rr.expected(sd, lp, b, tw)[0].cls)


# ---- the life of modes and field -----------------------------------------------------------------------------------------------------
def test_life(hiplib):
    sd, lp, S = vr.scene()
    zero = np.zeros_like(S.rest)
    g = _scene()
    want = _posed_twice(g)
    _check(g.render(_lp())[0], None, want, "mode after the table", populated=8)
    # the table after the mode: the same render
    t = _scene(table_first=False)
    _posed_twice(t)
    ht, rec, _ = t.render(_lp(), records=True)
    _check(ht, rec, want, "table after the mode", populated=8).check_two(ht, g.render(_lp())[0], "table after the mode against mode after the table")
    # a rebuild changes the slot order and carries the rows along
    g.rebuild_bvh()
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, want, "after rebuild_bvh", populated=8)
    # a clone keeps modes, dt and field; what the parent does afterwards does not reach it
    c = g.clone()
    assert c.get_velocity_mode(S.k) == (DIFF, vr.DT)
    g.pose_skin(S.k, _bones()[3])
    _check(g.render(_lp())[0], None, _exp(_P(3), _cv(_P(1), _P(3))), "the parent after another pose")
    h, rec, _ = c.render(_lp(), records=True)
    _check(h, rec, want, "the clone", populated=8)
    c.pose_skin(S.k, _bones()[2])
    _check(c.render(_lp())[0], None, _exp(_P(2), _cv(_P(1), _P(2))), "the clone's own next pose", populated=8)
    c.close()
    # mode back to BF_VELOCITY_TWIST: the twist alone again, bit for bit in every path, and the mode that follows starts from zero
    g.set_velocity_mode(S.k, TWIST)
    assert g.get_velocity_mode(S.k) == (TWIST, 0.0)
    plain = capi.Scene(sd)
    plain.set_skin(S.k, S.n_bones, S.rest, S.index, S.weight)
    plain.set_range_rate_classes(vr.table(), vr.still(sd))
    plain.pose_skin(S.k, _bones()[3])
    e0 = _exp(_P(3), zero)
    h, rec, _ = g.render(_lp(), records=True)
    hp, recp, _ = plain.render(_lp(), records=True)
    _same_records(rec, recp)
    _check(h, rec, e0, "back in BF_VELOCITY_TWIST", populated=0).check_two(h, hp, "against a handle that never left it")
    g.set_velocity_mode(S.k, DIFF, vr.DT)
    _check(g.render(_lp())[0], None, e0, "BF_VELOCITY_DIFFERENCE again: zero until the next move", populated=0)


def test_refusals_leave_the_scene_intact(hiplib):
    sd, lp, S = vr.scene()
    g = _scene()
    want = _posed_twice(g)
    lib, INVALID = hiplib, capi.BF_ERR_INVALID
    msg = lambda: (lib.bf_last_error() or b"").decode()
    nan, inf = float("nan"), float("inf")
    assert lib.bf_scene_set_velocity_mode(None, S.k, DIFF, 1.0) == INVALID and "null scene" in msg()
    assert lib.bf_scene_set_velocity_mode(g.handle, 0, DIFF, 1.0) == INVALID and "not a mesh" in msg()           # a rectangle
    assert lib.bf_scene_set_velocity_mode(g.handle, len(sd.shapes), DIFF, 1.0) == INVALID and "shapes" in msg()
    assert lib.bf_scene_set_velocity_mode(g.handle, S.k, 3, 1.0) == INVALID and "unknown mode 3" in msg()
    for dt in (0.0, -1.0, nan, inf):
        assert lib.bf_scene_set_velocity_mode(g.handle, S.k, DIFF, dt) == INVALID and "finite and positive" in msg(), dt
    V = np.zeros_like(S.rest)
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*not in BF_VELOCITY_VERTEX"):
        g.set_vertex_velocities(S.k, V)                      # the shape is in BF_VELOCITY_DIFFERENCE
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*not in BF_VELOCITY_VERTEX"):
        g.set_vertex_velocities(S.k - 1, None)               # the bus is in BF_VELOCITY_TWIST
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*not in BF_VELOCITY_VERTEX"):
        g.set_vertex_velocities(S.k, 16, device=True)
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*not a mesh"):
        g.set_vertex_velocities(0, None)
    assert lib.bf_scene_set_vertex_velocities(None, S.k, None, None) == INVALID and "null scene" in msg()
    assert lib.bf_scene_get_velocity_mode(g.handle, S.k, None, None) == INVALID and "null argument" in msg()
    # a batch of one render cannot difference anything
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*n_renders is 1.*BF_VELOCITY_DIFFERENCE"):
        g.render_skin_batch(_lp(), {S.k: _bones()[:1]})
    # a field with a value that is not finite: refused by the host form
    g.set_velocity_mode(S.k - 1, VERTEX)
    bad = np.zeros((int(sd.shapes[S.k - 1].n_vertices), 3), f32)
    bad[7, 1] = nan
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*non-finite value at vertex 7"):
        g.set_vertex_velocities(S.k - 1, bad)
    g.set_velocity_mode(S.k - 1, TWIST)
    # everything existing class launches are refused for keeps its status and message
    with pytest.raises(capi.BeifongError, match=rf"status {INVALID}\).*BF_FLAG_CLASSES.*BF_FLAG_FAST"):
        g.render(cr.classed(lp, capi.BF_FLAG_FAST))
    h, rec, _ = g.render(_lp(), records=True)
    _check(h, rec, want, "after the refusals", populated=8)
    assert g.get_velocity_mode(S.k) == (DIFF, vr.DT)


# ---- against the twist that states the same motion -----------------------------------------------------------------------------------
def test_translation_against_the_twist(hiplib):
    """the bar stepped by dx between two versions, differenced over dt, against BF_VELOCITY_TWIST under lin = dx / dt: where no
    path's rate lies within 1e-5 m/s of a bin edge under either model, both renders meet the same expected blocks"""
    sd, lp, S = vr.scene()
    dx, dt = np.array([-1 / 32, 1 / 128, 0.0], f32), vr.DT
    P1 = (S.rest + dx).astype(f32)
    V = _cv(S.rest, P1, dt)
    tw = vr.still(sd)
    tw[S.k] = motion.twist(lin=dx / f32(dt))
    on = motion.deformed_description(sd, {S.k: P1})
    bins = capi.range_rate_bins((-2.5, -1.5), 8)            # around dx / dt seen from the radar: about -2 m/s
    _, (d, p, shape, prim, uv, U, has) = vr.classes(sd, lp, bins, vr.still(sd), {S.k: V}, trace_sd=on)
    r_field = capi.range_rates(d, p, shape, bins, vr.still(sd), U, has).astype(np.float64)
    r_twist = capi.range_rates(d, p, shape, bins, tw).astype(np.float64)
    bar = shape == S.k
    assert bar.sum() > 500 and np.abs(r_field[bar] - r_twist[bar]).max() <= 1e-6      # (measured: 2.4e-7)
    edges = -2.5 + np.arange(9) / 8.0
    for r in (r_field[bar], r_twist[bar]):
        assert np.abs(r[:, None] - edges[None, :]).min() > 1e-5
    by_field, by_twist = _exp(P1, V, bins=bins), _exp(P1, np.zeros_like(V), bins=bins, twists=tw)
    assert np.array_equal(by_field[0].cls, by_twist[0].cls) and (by_field[0].population()[:8] > 0).sum() >= 2
    xf = np.tile(motion.rigid(), (2, len(sd.shapes), 1, 1)).astype(f32)
    xf[1, S.k] = motion.rigid(t=dx)
    g = capi.Scene(sd)
    g.set_range_rate_classes(bins, vr.still(sd))
    g.set_velocity_mode(S.k, DIFF, dt)
    hb, rb, _ = g.render_motion_batch(_lp(), xf, records=True)
    _check(hb[1], rb[1], by_field, "differenced translation", populated=2)
    t = capi.Scene(sd)
    t.set_range_rate_classes(bins, tw)
    t.set_velocity_mode(S.k, TWIST)
    ht, rt, _ = t.render_motion_batch(_lp(), xf, records=True)
    _check(ht[1], rt[1], by_field, "the twist lin = dx / dt", populated=2).check_two(hb[1], ht[1], "differenced against twisted")


# ---- BF_VELOCITY_TWIST: the range-rate tests' scenes as they were --------------------------------------------------------------------
@pytest.mark.parametrize("scene", ["receive", "film", "global"])
def test_mode_0_is_unchanged(hiplib, scene):
    """every scene of tests/test_gpu_range_rate.py, its meshes set to BF_VELOCITY_TWIST by name (and, once, through another mode
    and back): the expected blocks of the twists alone"""
    from beifong_amd import scenes
    twin = None
    if scene == "receive":
        sd, lp = cr.receive_scene(4096)
        twin, name = cr.fluxmeter_twin(cr.receive_scene), "narrow"
    elif scene == "film":
        (sd, lp), name = cr.film_scene(), "film"
    else:
        (sd, lp), name = scenes.bus_radar(n_tris=2000, n_paths=4096, bins=2560, dr=0.01, seed=7), "global"
    exp, rec_o, _ = rr.expected(sd, lp, rr.table(name), rr.twists(sd), twin=twin)
    pop = exp.population()
    assert (pop[:-2].tolist(), int(pop[-2]), int(pop[-1])) == rr.POPULATIONS[(scene, name)]
    k = len(sd.shapes) - 1
    g = capi.Scene(sd)
    g.set_velocity_mode(k, TWIST)
    g.set_range_rate_classes(rr.table(name), rr.twists(sd))
    h, rec, _ = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    exp.check(h, f"{scene}: BF_VELOCITY_TWIST")
    g.set_velocity_mode(k, VERTEX)
    g.set_velocity_mode(k, TWIST)
    h2, rec, _ = g.render(cr.classed(lp), records=True)
    _same_records(rec, rec_o)
    exp.check(h2, f"{scene}: through BF_VELOCITY_VERTEX and back")
    exp.check_two(h, h2, f"{scene}: the two renders")
