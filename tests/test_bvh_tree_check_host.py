"""The checker of tests/bvh_tree_check.py has to be able to fail: a tiny four-wide and a tiny sixteen-wide tree built by hand in
numpy (five triangles, one node, three leaf children, one unused slot), padded by the rule, with one Node4Q encoded beside the
four-wide node.  check_padding, check_quantised and the origin-scale bracket accept them and reject each single corruption a
subtly wrong translate, refit or requantise kernel would produce, with a message that names the violated rule.

No library and no GPU: this is the evidence, checkable on any machine, that tests/test_gpu_refit_trees.py would notice."""
import math

import numpy as np
import pytest

from beifong_amd import capi
from tests import bvh_tree_check as tc

f32 = np.float32
S = f32(12.5)                      # the origin scale the hand-made trees are padded for
LEAVES = [(0, 2), (2, 2), (4, 1)]  # (first triangle, count) of the three leaf children


def _rows():
    rng = np.random.default_rng(5)
    rows = np.zeros((5, 3, 4), f32)
    rows[:, :, :3] = (rng.uniform(-1.0, 1.0, (5, 1, 3)) * 3.0 + rng.uniform(-0.2, 0.2, (5, 3, 3))).astype(f32)
    w = rows.view(np.uint32)
    w[:, 0, 3] = np.arange(5)          # prim
    w[:, 1, 3] = 0                     # shape
    return rows


def _leaf_ref(first, count, width):
    shift = 3 if width == 4 else 4
    return np.int32(~((first << shift) | (count - 1)))


def _tree(width, rows, pad):
    """one node over LEAVES, padded by pad(ulo, uhi) -> (lo, hi)"""
    nodes = np.zeros(1, capi.NODE4_DTYPE if width == 4 else capi.NODE16_DTYPE)
    lo, hi = np.full((width, 3), np.inf, f32), np.full((width, 3), -np.inf, f32)
    ref = np.full(width, tc.EMPTY, np.int32)
    for k, (first, count) in enumerate(LEAVES):
        p = rows[first:first + count, :, :3].reshape(-1, 3)
        lo[k], hi[k] = pad(p.min(0), p.max(0))
        ref[k] = _leaf_ref(first, count, width)
    _store(nodes, width, lo, hi, ref)
    return nodes


def _store(nodes, width, lo, hi, ref):
    if width == 4:
        for a, name in enumerate("xyz"):
            nodes["lo" + name][0], nodes["hi" + name][0] = lo[:, a], hi[:, a]
        nodes["child"][0] = ref
    else:
        nodes["c"]["lo"][0], nodes["c"]["hi"][0], nodes["c"]["child"][0] = lo, hi, ref


def _boxes(nodes, width):
    lo, hi, ref = tc._children(nodes, width)
    return lo[0].copy(), hi[0].copy(), ref[0].copy()


def _refit(rows, width, scale=S):
    return _tree(width, rows, lambda a, b: tc.refit_pad(a, b, scale))


def _quantise(nodes):
    """bf::quantise_node4 / quantise_node4_dev for one node, in numpy float32"""
    lo, hi, ref = _boxes(nodes, 4)
    used = ref != tc.EMPTY
    q = np.zeros(1, tc.NODE4Q_DTYPE)
    q["child"][0] = ref
    exps = 0
    for a in range(3):
        nlo, nhi = lo[used, a].min(), hi[used, a].max()
        _, e = math.frexp(float((nhi - nlo) * (f32(1.0) / f32(255.0))))
        e = max(-100, min(100, e))
        if not (nlo + f32(255.0) * f32(2.0 ** e) >= nhi):
            e += 1
        s = f32(2.0 ** e)
        exps |= (e + 127) << (8 * a)
        ql_w = qh_w = 0
        for k in range(4):
            ql, qh = 255, 0
            if used[k]:
                ql = int(min(255.0, max(0.0, math.floor(float((lo[k, a] - nlo) * (f32(1.0) / s))))))
                qh = int(min(255.0, max(0.0, math.ceil(float((hi[k, a] - nlo) * (f32(1.0) / s))))))
                while ql > 0 and nlo + f32(ql) * s > lo[k, a]:
                    ql -= 1
                while qh < 255 and nlo + f32(qh) * s < hi[k, a]:
                    qh += 1
            ql_w |= ql << (8 * k)
            qh_w |= qh << (8 * k)
        q["lo"][0, a], q["qlo"][0, a], q["qhi"][0, a] = nlo, ql_w, qh_w
    q["exps"][0] = exps
    return q


def _ulp_in(x, towards):
    return np.nextafter(f32(x), f32(towards))


@pytest.mark.parametrize("width", [4, 16])
def test_the_hand_made_trees_pass(width):
    rows = _rows()
    nodes = _refit(rows, width)
    root = 0
    assert tc.check_tree(nodes, rows, root, width)[2] == 1
    tc.check_padding(nodes, rows, width, S, "refit")
    d = np.array([0.3, 300.0, -1e4], f32)
    moved = rows.copy()
    moved[:, :, :3] += d
    lo0, hi0, ref = _boxes(nodes, width)
    t = nodes.copy()
    used = ref != tc.EMPTY
    lo, hi = lo0.copy(), hi0.copy()
    lo[used], hi[used] = tc.translate_pad(lo0[used], hi0[used], d)
    _store(t, width, lo, hi, ref)
    tc.check_tree(t, moved, root, width)
    tc.check_padding(t, moved, width, S, "translate", before=(nodes, rows), offset=d)
    if width == 4:
        tc.check_quantised(_quantise(nodes), nodes)
        tc.check_quantised(_quantise(t), t)


@pytest.mark.parametrize("width", [4, 16])
def test_a_face_one_ulp_inward_is_rejected(width):
    rows = _rows()
    for side in ("lo", "hi"):
        nodes = _refit(rows, width)
        lo, hi, ref = _boxes(nodes, width)
        if side == "lo":
            lo[1, 2] = _ulp_in(lo[1, 2], np.inf)
        else:
            hi[2, 0] = _ulp_in(hi[2, 0], -np.inf)
        _store(nodes, width, lo, hi, ref)
        tc.check_tree(nodes, rows, 0, width)          # still a valid tree: only the padding contract sees it
        with pytest.raises(AssertionError, match="refit_pad"):
            tc.check_padding(nodes, rows, width, S, "refit")


@pytest.mark.parametrize("width", [4, 16])
def test_a_box_padded_twice_is_rejected(width):
    rows = _rows()
    nodes = _refit(rows, width)
    lo, hi, ref = _boxes(nodes, width)
    lo[0], hi[0] = tc.refit_pad(lo[0], hi[0], S)
    _store(nodes, width, lo, hi, ref)
    tc.check_tree(nodes, rows, 0, width)
    with pytest.raises(AssertionError, match="refit_pad"):
        tc.check_padding(nodes, rows, width, S, "refit")
    # the same under the translation rule: a box shifted from an already shifted box
    d = np.array([0.3, -0.2, 0.05], f32)
    base = _refit(rows, width)
    lo0, hi0, ref = _boxes(base, width)
    used = ref != tc.EMPTY
    lo, hi = lo0.copy(), hi0.copy()
    lo[used], hi[used] = tc.translate_pad(*tc.translate_pad(lo0[used], hi0[used], d * f32(0.5)), d * f32(0.5))
    t = base.copy()
    _store(t, width, lo, hi, ref)
    moved = rows.copy()
    moved[:, :, :3] += d
    with pytest.raises(AssertionError, match="bf_translate_kernel"):
        tc.check_padding(t, moved, width, S, "translate", before=(base, rows), offset=d)


@pytest.mark.parametrize("width", [4, 16])
def test_a_nan_unused_slot_is_rejected(width):
    rows = _rows()
    nodes = _refit(rows, width)
    lo, hi, ref = _boxes(nodes, width)
    with np.errstate(invalid="ignore"):
        e = f32(2.4e-7) * np.maximum(np.abs(lo[3]), np.abs(hi[3]))       # what shifting an inverted box computes: inf - inf
        lo[3], hi[3] = lo[3] - e, hi[3] + e
    assert np.isnan(lo[3]).all() and np.isnan(hi[3]).all()
    _store(nodes, width, lo, hi, ref)
    with pytest.raises(AssertionError, match="unused slot holds NaN"):
        tc.check_padding(nodes, rows, width, S, "refit")
    with pytest.raises(AssertionError, match="unused slot"):
        tc.check_tree(nodes, rows, 0, width)


@pytest.mark.parametrize("width", [4, 16])
def test_an_origin_scale_too_small_is_rejected(width):
    rows = _rows()
    nodes = _refit(rows, width, f32(0.9) * S)
    tc.check_tree(nodes, rows, 0, width)
    with pytest.raises(AssertionError, match="origin_scale"):
        tc.check_padding(nodes, rows, width, S, "refit")
    # and the bracket itself: 10 % below the largest coordinate, 10 % above the documented bound
    tc.check_origin_scale(f32(12.5), (12.5, 12.5))
    tc.check_origin_scale(f32(12.5), (10.0, 20.0))
    with pytest.raises(AssertionError, match="too small"):
        tc.check_origin_scale(f32(0.9 * 12.5), (12.5, 20.0))
    with pytest.raises(AssertionError, match="exceeds the documented bound"):
        tc.check_origin_scale(f32(1.1 * 20.0), (12.5, 20.0))


def test_a_quantised_plane_one_step_inside_is_rejected():
    rows = _rows()
    nodes = _refit(rows, 4)
    good = _quantise(nodes)
    tc.check_quantised(good, nodes)
    lo, hi, scale, ql, qh = tc.decode_node4q(good)
    # a lower plane that can move up by one step (it is not at 255), an upper plane that can move down by one
    for field, k, a, step in (("qlo", 1, 0, 1), ("qhi", 2, 1, -1)):
        q = good.copy()
        byte = (int(q[field][0, a]) >> (8 * k)) & 0xff
        assert 0 <= byte + step <= 255
        q[field][0, a] = (int(q[field][0, a]) & ~(0xff << (8 * k))) | ((byte + step) << (8 * k))
        with pytest.raises(AssertionError, match="inside the fp32 box"):
            tc.check_quantised(q, nodes)
    q = good.copy()                                   # one step OUTSIDE twice over: more than a quantum of growth
    byte = (int(q["qhi"][0, 2]) >> 8) & 0xff
    if byte + 2 <= 255:
        q["qhi"][0, 2] = (int(q["qhi"][0, 2]) & ~(0xff << 8)) | ((byte + 2) << 8)
        with pytest.raises(AssertionError, match="more than one quantum"):
            tc.check_quantised(q, nodes)
    q = good.copy()
    q["qlo"][0, 0] = int(q["qlo"][0, 0]) & 0x00ffffff  # the unused slot's lower byte 0 instead of 255
    with pytest.raises(AssertionError, match="does not decode inverted"):
        tc.check_quantised(q, nodes)
    q = good.copy()
    q["child"][0, 0] = 7
    with pytest.raises(AssertionError, match="references differ"):
        tc.check_quantised(q, nodes)


@pytest.mark.parametrize("width", [4, 16])
def test_a_row_one_ulp_off_is_rejected(width):
    rows = _rows()
    base = _refit(rows, width)
    d = np.array([0.3, -0.2, 0.05], f32)
    lo0, hi0, ref = _boxes(base, width)
    used = ref != tc.EMPTY
    lo, hi = lo0.copy(), hi0.copy()
    lo[used], hi[used] = tc.translate_pad(lo0[used], hi0[used], d)
    t = base.copy()
    _store(t, width, lo, hi, ref)
    moved = rows.copy()
    moved[:, :, :3] += d
    tc.check_padding(t, moved, width, S, "translate", before=(base, rows), offset=d)
    bad = moved.copy()
    bad[3, 1, 2] = _ulp_in(bad[3, 1, 2], np.inf)
    with pytest.raises(AssertionError, match=r"fl\(v0 \+ d\)"):
        tc.check_padding(t, bad, width, S, "translate", before=(base, rows), offset=d)
    bad = moved.copy()
    bad.view(np.uint32)[2, 0, 3] ^= 1                 # a .w word changed
    with pytest.raises(AssertionError, match=r"fl\(v0 \+ d\)"):
        tc.check_padding(t, bad, width, S, "translate", before=(base, rows), offset=d)


def test_origin_scale_bounds_from_a_description():
    from beifong_amd import meshgen, motion, scenes
    v, f = meshgen.triangle_soup(17, seed=4)
    sd = scenes.single_mesh(v, f)
    s_lo, s_hi = tc.origin_scale_bounds(sd)
    assert s_lo == s_hi == float(np.abs(v).max())
    far = np.stack([motion.rigid(t=(2000.0, 0.0, 0.0))])
    lo2, hi2 = tc.origin_scale_bounds(sd, [far])
    vmax = np.abs(v.astype(np.float64)).max(0)
    assert lo2 == s_lo and hi2 == (2000.0 + vmax[0]) * (1 + 1e-5)
    assert tc.origin_scale_bounds(sd, [np.stack([motion.rigid()])]) == (s_lo, s_hi)      # the identity moves nothing
    lo3, hi3 = tc.origin_scale_bounds(sd, [{"xf": np.stack([motion.rigid()]), "all": True, "boxes": {0: ([-9, -9, -9], [9, 9, 9])}}])
    assert lo3 == s_lo and hi3 == 9.0 * (1 + 1e-5)
