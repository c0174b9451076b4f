"""Pure-numpy walker over the arrays capi.Scene.read_bvh returns: the contract every device tree must meet, whoever built it
(the host builder of bf_scene_create or the device builder of bf_scene_rebuild_bvh).

For width 4 and width 16: every triangle slot lies in exactly one leaf; leaves hold at most 2 (16) triangles; every child box
contains the boxes and triangles beneath it; unused slots are inverted with kEmptyChild; the width-4 prefix of min(85, n)
nodes is breadth-first; the recomputed depth and stack need equal bf_scene_get_info's (width 4) and lie within the bounds
tests/test_bvh_host.py states (binary depth <= 31, four-wide stack <= 93, sixteen-wide stack <= 512).

For what a translate, a refit or a requantise writes (tests/test_gpu_refit_trees.py) three more checks, each a restatement of a
documented rule and none with a tolerance of its own:
  check_padding        every used box equals, bit for bit, the exact union of the triangle rows beneath it padded by the rule of the
                       call that wrote it (bf_geom.hip: refit_pad / bf_translate_kernel, every operation a singly rounded float32
                       one, which numpy float32 reproduces); unused slots are exactly (+inf, -inf)
  check_quantised      the Node4Q array against the fp32 nodes, by the contract tests/test_bvh_host.py states for the host quantiser
  origin_scale_bounds  a float64 bracket, from the description and the poses a handle was given, for the ray-origin bound the boxes
                       are padded for
tests/test_bvh_tree_check_host.py shows on hand-made trees that each of them can fail."""
import numpy as np

f32 = np.float32

EMPTY = -(1 << 31)
K_TOP = 85


def _children(nodes, width):
    """(lo [n, W, 3], hi [n, W, 3], ref [n, W])"""
    if width == 4:
        lo = np.stack([nodes["lox"], nodes["loy"], nodes["loz"]], -1)
        hi = np.stack([nodes["hix"], nodes["hiy"], nodes["hiz"]], -1)
        return lo, hi, nodes["child"]
    c = nodes["c"]
    return c["lo"], c["hi"], c["child"]


def _leaf(ref, width):
    enc = ~int(ref) & 0xffffffff
    shift, mask = (3, 7) if width == 4 else (4, 15)
    return enc >> shift, (enc & mask) + 1


def check_tree(nodes, rows, root, width, info=None):
    """Walk the tree level by level; returns (depth, stack_need, n_nodes).  `rows`: float32[n, 3, 4]."""
    n_tris = rows.shape[0]
    max_leaf = 2 if width == 4 else 16
    if n_tris == 0:
        return 0, 0, 0
    tlo, thi = rows[:, :, :3].min(1), rows[:, :, :3].max(1)
    covered = np.zeros(n_tris, np.int64)
    if root < 0:
        assert root != EMPTY, "no root"
        f, c = _leaf(root, width)
        assert f == 0 and c == n_tris and c <= max_leaf, (f, c, n_tris)
        assert len(nodes) == 0
        return 0, 0, 0
    assert root == 0
    lo, hi, ref = _children(nodes, width)
    n = len(nodes)
    used = ref != EMPTY
    # unused slots: inverted boxes
    assert np.all(lo[~used] == np.inf) and np.all(hi[~used] == -np.inf), "an unused slot is not inverted"
    assert np.all(np.isfinite(lo[used])) and np.all(np.isfinite(hi[used]))
    assert np.all(used[:, :2].all(1)), "a node with fewer than two children"
    # the box of everything beneath each node, bottom-up over breadth-first levels
    level = np.array([0], np.int64)
    levels, seen = [], np.zeros(n, bool)
    order_bfs = []
    need = np.zeros(n, np.int64)
    kids = used.sum(1)
    need[0] = kids[0] - 1 if width == 4 else kids[0]
    while level.size:
        assert not seen[level].any(), "a node is referenced twice"
        seen[level] = True
        levels.append(level)
        order_bfs.append(level)
        r = ref[level]
        internal = (r >= 0) & (r != EMPTY)
        par = np.repeat(level, internal.sum(1))
        nxt = r[internal].astype(np.int64)
        assert np.all(nxt < n)
        need[nxt] = need[par] + (kids[nxt] - 1 if width == 4 else kids[nxt])
        level = nxt
    assert seen.all(), f"{(~seen).sum()} nodes are unreachable"
    depth = len(levels)
    stack_need = int(need.max())
    # leaves: coverage and containment of the triangles
    is_leaf = used & (ref < 0)
    lr = ref[is_leaf].astype(np.int64)
    enc = (~lr) & 0xffffffff
    shift, mask = (3, 7) if width == 4 else (4, 15)
    first, count = enc >> shift, (enc & mask) + 1
    assert np.all(count <= max_leaf), f"a leaf of {count.max()} triangles"
    assert np.all(first + count <= n_tris)
    llo, lhi = lo[is_leaf], hi[is_leaf]
    for j in range(max_leaf):
        m = count > j
        t = first[m] + j
        np.add.at(covered, t, 1)
        assert np.all(llo[m] <= tlo[t]) and np.all(lhi[m] >= thi[t]), "a leaf box does not contain its triangle"
    assert np.all(covered == 1), f"{(covered != 1).sum()} triangle slots are not in exactly one leaf"
    # internal children: the child's box contains the union of the boxes inside the child node
    ulo = np.where(used[..., None], lo, np.inf).min(1)
    uhi = np.where(used[..., None], hi, -np.inf).max(1)
    internal = used & (ref >= 0)
    ci = ref[internal].astype(np.int64)
    assert np.all(lo[internal] <= ulo[ci]) and np.all(hi[internal] >= uhi[ci]), "a child box does not contain the boxes beneath it"
    if width == 4:
        # the prefix is breadth-first: node i of the first min(85, n) is the i-th node of a breadth-first walk
        bfs = np.concatenate(order_bfs)[: min(K_TOP, n)]
        assert np.array_equal(bfs, np.arange(len(bfs))), "the first nodes are not the top levels in breadth-first order"
        assert depth <= 31 and stack_need <= 93, (depth, stack_need)
        if info is not None:
            assert info.n_bvh_nodes == n and info.bvh_depth == depth and info.bvh_stack_need == stack_need, \
                (info.n_bvh_nodes, n, info.bvh_depth, depth, info.bvh_stack_need, stack_need)
    else:
        assert stack_need <= 512 and 16 * depth <= 512, (depth, stack_need)
    return depth, stack_need, n


def prim_shape_multiset(rows):
    w = rows.view(np.uint32)
    keys = (w[:, 1, 3].astype(np.uint64) << np.uint64(32)) | w[:, 0, 3].astype(np.uint64)
    return np.sort(keys)


def check_scene(scene, before=None):
    """Both trees of a capi.Scene; `before`: prim_shape_multiset of the rows before a rebuild.  Returns the rows' multiset."""
    info = scene.info()
    nodes, rows, root = scene.read_bvh(4)
    check_tree(nodes, rows, root, 4, info)
    try:
        wn, wrows, wroot = scene.read_bvh(16)
    except Exception as e:
        if "sixteen-wide" not in str(e):
            raise
    else:
        assert np.array_equal(wrows.view(np.uint32), rows.view(np.uint32))
        check_tree(wn, wrows, wroot, 16)
    ms = prim_shape_multiset(rows)
    if before is not None:
        assert np.array_equal(ms, before), "the rows' (prim, shape) words changed"
    return ms


# ---- the padding contract ----------------------------------------------------------------------------------------------------------
def _levels(ref):
    """node indices by breadth-first level from node 0"""
    out, level = [], np.array([0], np.int64)
    while level.size:
        out.append(level)
        r = ref[level]
        level = r[(r >= 0)].astype(np.int64)
        assert len(out) <= 64, "the tree is deeper than any builder makes it (a reference cycle?)"
    return out


def child_unions(nodes, rows, width):
    """(ulo, uhi) [n, W, 3] float32: for every child slot the exact union (min / max only) of the triangle rows beneath it;
    (+inf, -inf) for unused slots."""
    _, _, ref = _children(nodes, width)
    n, W = ref.shape
    ulo = np.full((n, W, 3), np.inf, f32)
    uhi = np.full((n, W, 3), -np.inf, f32)
    if n == 0:
        return ulo, uhi
    tlo, thi = rows[:, :, :3].min(1), rows[:, :, :3].max(1)
    shift, mask = (3, 7) if width == 4 else (4, 15)
    is_leaf = (ref < 0) & (ref != EMPTY)
    enc = (~ref[is_leaf].astype(np.int64)) & 0xffffffff
    first, count = enc >> shift, (enc & mask) + 1
    llo = np.full((first.size, 3), np.inf, f32)
    lhi = np.full((first.size, 3), -np.inf, f32)
    for j in range(int(count.max()) if count.size else 0):
        m = count > j
        llo[m] = np.minimum(llo[m], tlo[first[m] + j])
        lhi[m] = np.maximum(lhi[m], thi[first[m] + j])
    ulo[is_leaf], uhi[is_leaf] = llo, lhi
    for level in reversed(_levels(ref)):
        r = ref[level]
        internal = r >= 0
        c = r[internal].astype(np.int64)
        sub_lo, sub_hi = ulo[level], uhi[level]
        sub_lo[internal], sub_hi[internal] = ulo[c].min(1), uhi[c].max(1)      # (the level below is complete)
        ulo[level], uhi[level] = sub_lo, sub_hi
    return ulo, uhi


def refit_pad(ulo, uhi, origin_scale):
    """bf_geom.hip: refit_pad == bf_bvh.cpp: Builder::pad of an unpadded box [..., 3], in float32, every operation rounded singly:
    m = max over axes of max(hi - lo, |lo|, |hi|);  e = 2e-6f m + (2e-7f origin_scale) + 1e-30f;  (lo - e, hi + e)"""
    ulo, uhi = np.asarray(ulo, f32), np.asarray(uhi, f32)
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.maximum(np.maximum(uhi - ulo, np.maximum(np.abs(ulo), np.abs(uhi))).max(-1), f32(0))
        abs_pad = f32(2e-7) * f32(origin_scale)
        e = ((f32(2e-6) * m + abs_pad) + f32(1e-30))[..., None]
        return (ulo - e).astype(f32), (uhi + e).astype(f32)


def translate_pad(lo0, hi0, d):
    """bf_geom.hip: bf_translate_kernel's box rule, in float32: lo' = fl(lo0 + d), hi' = fl(hi0 + d),
    e = fl(2.4e-7f max(|lo'|, |hi'|)) per axis; (lo' - e, hi' + e)"""
    d = np.asarray(d, f32).reshape(3)
    with np.errstate(invalid="ignore"):
        lo, hi = np.asarray(lo0, f32) + d, np.asarray(hi0, f32) + d
        e = f32(2.4e-7) * np.maximum(np.abs(lo), np.abs(hi))
        return (lo - e).astype(f32), (hi + e).astype(f32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def check_padding(nodes, rows, width, origin_scale, rule, before=None, offset=None):
    """The boxes of `nodes` (width 4 or 16) over the rows float32[n, 3, 4] against the rule of the call that wrote them.
    rule="refit": `origin_scale` is the bound the handle reports after the call.
    rule="translate": before = (nodes, rows) read from the handle's geometry as created, offset = the call's offset."""
    lo, hi, ref = _children(nodes, width)
    used = ref != EMPTY
    assert not np.isnan(lo[~used]).any() and not np.isnan(hi[~used]).any(), "an unused slot holds NaN: unused slots are exactly (+inf, -inf)"
    assert np.all(lo[~used] == np.inf) and np.all(hi[~used] == -np.inf), "an unused slot is not exactly (+inf, -inf)"
    if rule == "translate":
        nodes0, rows0 = before
        d = np.asarray(offset, f32).reshape(3)
        want_rows = rows0.copy()
        want_rows[:, :, :3] = rows0[:, :, :3] + d
        assert np.array_equal(_bits(rows), _bits(want_rows)), "a triangle row is not fl(v0 + d) with its .w word kept"
    ulo, uhi = child_unions(nodes, rows, width)
    if rule == "refit":
        wlo, whi = refit_pad(ulo, uhi, origin_scale)
        what = "the union of its rows padded by 2e-6 m + 2e-7 origin_scale + 1e-30 (refit_pad)"
    elif rule == "translate":
        lo0, hi0, ref0 = _children(nodes0, width)
        assert np.array_equal(ref0, ref), "the child references changed"
        wlo, whi = translate_pad(lo0, hi0, d)
        what = "its box as created shifted by d and padded by 2.4e-7 of its largest shifted coordinate (bf_translate_kernel)"
    else:
        raise ValueError(rule)
    if used.any():
        bad = used & ((_bits(lo) != _bits(wlo)) | (_bits(hi) != _bits(whi))).any(-1)
        if bad.any():
            i, k = np.argwhere(bad)[0]
            raise AssertionError(f"{int(bad.sum())} used boxes of the {width}-wide tree are not {what}: node {i} slot {k} holds "
                                 f"lo {lo[i, k]!r} hi {hi[i, k]!r}, the rule gives lo {wlo[i, k]!r} hi {whi[i, k]!r} (origin scale {origin_scale!r})")
        assert np.all(lo[used] < ulo[used]) and np.all(hi[used] > uhi[used]), \
            "a used box does not strictly contain the rows beneath it: no positive margin on some axis"


# ---- the quantised nodes -----------------------------------------------------------------------------------------------------------
NODE4Q_DTYPE = np.dtype([("lo", "<f4", (3,)), ("exps", "<u4"), ("child", "<i4", (4,)), ("qlo", "<u4", (3,)), ("qhi", "<u4", (3,)),
                         ("pad", "<u4", (2,))])


def decode_node4q(q):
    """(lo, hi [n, 4, 3] float32, scale [n, 3] float32, ql, qh [n, 4, 3]): the child planes as the kernels evaluate them
    (bf_bvh.h: lo_a + q 2^(e_a - 127), in float32: the byte times a power of two is exact, the sum is rounded once)"""
    ax = np.arange(3, dtype=np.uint32)
    e = (q["exps"][:, None] >> (8 * ax)[None, :]) & 0xff                                  # [n, 3]
    scale = (e.astype(np.uint32) << 23).view(f32)
    k = (8 * np.arange(4, dtype=np.uint32))[None, :, None]
    ql = ((q["qlo"][:, None, :] >> k) & 0xff).astype(f32)                                  # [n, 4, 3]
    qh = ((q["qhi"][:, None, :] >> k) & 0xff).astype(f32)
    base = q["lo"][:, None, :]
    return (base + ql * scale[:, None, :]).astype(f32), (base + qh * scale[:, None, :]).astype(f32), scale, ql, qh


def check_quantised(qnodes, nodes):
    """tests/test_bvh_host.py::test_quantised_nodes_contain_the_fp32_boxes, for the Node4Q array a device kernel wrote: every
    decoded child box contains the fp32 box of the same slot and grows it by at most one quantum of the node (the host test's
    bound: 1.0001 s), that quantum being at most 2.01 / 255 of the node's extent (twice 1 / 255 where the extent sits just below
    a power of two); references equal; unused slots decode inverted (ql = 255, qh = 0)."""
    q = np.ascontiguousarray(qnodes).view(NODE4Q_DTYPE).reshape(-1)
    assert len(q) == len(nodes), (len(q), len(nodes))
    if len(q) == 0:
        return
    lo, hi, ref = _children(nodes, 4)
    assert np.array_equal(q["child"], ref), "a quantised node's child references differ from the fp32 node's"
    used = ref != EMPTY
    plo, phi, scale, ql, qh = decode_node4q(q)
    assert np.all(ql[~used] == 255) and np.all(qh[~used] == 0), "an unused slot of a quantised node does not decode inverted (ql = 255, qh = 0)"
    assert not np.isnan(q["lo"]).any() and np.all(scale > 0) and np.all(np.isfinite(scale)), "a quantised node's origin or scale is not a number"
    assert np.all(plo[used] <= lo[used]) and np.all(phi[used] >= hi[used]), "a quantised plane lies inside the fp32 box it replaces"
    s = np.broadcast_to(scale[:, None, :].astype(np.float64), lo.shape)
    grow = np.maximum(lo.astype(np.float64) - plo, phi.astype(np.float64) - hi)
    assert np.all(grow[used] <= 1.0001 * s[used]), "a quantised box grows its fp32 box by more than one quantum of the node"
    nlo = np.where(used[..., None], lo, np.inf).min(1)
    nhi = np.where(used[..., None], hi, -np.inf).max(1)
    ext = (nhi - nlo).astype(np.float64)
    free = ext / 255.0 > 2.0 ** -99                      # (the exponent is clamped to [-100, 100]: a flat node keeps 2^-100)
    assert np.all(scale[free] <= 2.01 / 255.0 * ext[free]), "a quantised node's quantum is more than 2 / 255 of its extent"


# ---- the ray-origin bound ------------------------------------------------------------------------------------------------------------
def origin_scale_bounds(sd, poses_seen=()):
    """(S_lo, S_hi) in float64 for the bound a handle of `sd` pads its boxes for.  S_lo: the largest |coordinate| of any sensor or
    emitter position, rectangle corner or mesh vertex of the description.  S_hi: S_lo raised, for every pose the handle has been
    given, by the bound bf_mesh.cpp: origin_bound documents: per row |t| + sum_c |R_rc| max(|box lo_c|, |box hi_c|), times
    1 + 1e-5.  An entry of `poses_seen` is a float[n_shapes, 3, 4] table (a transform call: a mesh whose entry is the identity is
    not moved and does not count) or a dict {"xf": table, "all": True, "boxes": {shape: (lo, hi)}}: "all" counts every mesh (the
    pose re-applied after a vertex update), "boxes" replaces the base box of those meshes from this entry on (a vertex update: the
    box of the new vertices, or [-bound, bound]^3 for the device form)."""
    from beifong_amd import capi
    pts, base = [np.asarray(sd.sensor.to_world, np.float64).reshape(4, 4)[:3, 3]], {}
    for e in sd.emitters:
        pts.append(np.asarray(e.to_world, np.float64).reshape(4, 4)[:3, 3])
    for k, s in enumerate(sd.shapes):
        if s.type == capi.BF_SHAPE_MESH:
            if s.n_vertices and s.n_faces:
                p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).astype(np.float64)
                base[k] = (p.min(0), p.max(0))
                pts.append(p)
        elif s.type == capi.BF_SHAPE_RECTANGLE:
            m = np.asarray(s.to_world, np.float64).reshape(4, 4)
            pts.append((np.array([[x, y, 0.0, 1.0] for x in (-1, 1) for y in (-1, 1)]) @ m.T)[:, :3])
    s_lo = s_hi = max(float(np.abs(p).max()) for p in pts)
    ident = np.hstack([np.eye(3), np.zeros((3, 1))])
    for entry in poses_seen:
        every = False
        if isinstance(entry, dict):
            for k, (blo, bhi) in entry.get("boxes", {}).items():
                base[int(k)] = (np.asarray(blo, np.float64).reshape(3), np.asarray(bhi, np.float64).reshape(3))
            every, entry = bool(entry.get("all")), entry.get("xf")
        if entry is None:
            continue
        xf = np.asarray(entry, np.float32).astype(np.float64).reshape(len(sd.shapes), 3, 4)
        for k, (blo, bhi) in base.items():
            if not every and np.array_equal(xf[k], ident):
                continue
            v = np.abs(xf[k][:, 3]) + np.abs(xf[k][:, :3]) @ np.maximum(np.abs(blo), np.abs(bhi))
            s_hi = max(s_hi, float(v.max()) * (1.0 + 1e-5))
    return s_lo, s_hi


def check_origin_scale(S, bounds):
    s_lo, s_hi = bounds
    assert s_lo * (1 - 1e-6) <= S, f"the origin scale {S!r} is below the largest coordinate of the description, {s_lo!r}: too small (or lowered)"
    assert S <= s_hi * (1 + 1e-6), f"the origin scale {S!r} exceeds the documented bound over every pose seen, {s_hi!r}"
