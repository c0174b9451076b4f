"""Pure-numpy walker over the arrays capi.Scene.read_bvh returns: the contract every device tree must meet, whoever built it
(the host builder of bf_scene_create or the device builder of bf_scene_rebuild_bvh).

For width 4 and width 16: every triangle slot lies in exactly one leaf; leaves hold at most 2 (16) triangles; every child box
contains the boxes and triangles beneath it; unused slots are inverted with kEmptyChild; the width-4 prefix of min(85, n)
nodes is breadth-first; the recomputed depth and stack need equal bf_scene_get_info's (width 4) and lie within the bounds
tests/test_bvh_host.py states (binary depth <= 31, four-wide stack <= 93, sixteen-wide stack <= 512)."""
import numpy as np

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
