"""The host builder (bf_bvh.cpp) held to the split rule and the adoption rule of tests/sah_ref.py, on the CPU, through bvh_export of
tests/native/bvh_check.cpp; and the verifier shown to fail: on a builder compiled with eight bins, on a hand-made wrong grouping and on
a hand-made three-child node with an internal child.

The statistics asserted here (no forced and no coincident node on the soup and the bus, the cluster boundaries, forced cuts on the
spiral, coincident cuts on the soup with copies) were measured on the host builder; tests/test_gpu_build_splits.py holds the device
builder to the same inputs."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

from beifong_amd import capi, meshgen
from tests import sah_ref
from tests.bvh_tree_check import EMPTY, check_padding, check_tree, refit_pad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

CLUSTERS = {
    (64, 65): [(0, 129, 0), (0, 64, 1), (64, 65, 1)],
    (300, 212): [(0, 300, 1), (300, 212, 1)],
    (256, 256, 256, 257): [(0, 256, 2), (256, 256, 2), (512, 256, 2), (768, 257, 2)],
    (63, 64, 65, 66, 190, 320): [(0, 63, 3), (63, 64, 3), (127, 65, 3), (192, 66, 3), (258, 190, 2), (448, 320, 2)],
}


@functools.lru_cache(maxsize=None)
def mesh(name):
    """the inputs of this file and of tests/test_gpu_build_splits.py: (v, f), never modified"""
    if name == "soup3000":
        return meshgen.triangle_soup(3000, seed=3)
    if name == "bus6000":
        return meshgen.bus(6000, seed=1)
    if name == "spiral":
        return sah_ref.spiral(400)
    if name == "copies":
        return sah_ref.soup_with_copies(500, 40)
    if name.startswith("clusters"):
        return sah_ref.clusters([int(x) for x in name.split("_")[1:]])
    raise KeyError(name)


def cluster_name(sizes):
    return "clusters_" + "_".join(str(s) for s in sizes)


def check_cluster_nodes(sizes, rec):
    for node in CLUSTERS[tuple(sizes)]:
        assert node in rec.nodes, (sizes, node)


def _build(tmp_path_factory, name, flags):
    out = tmp_path_factory.mktemp(name) / "libbvh_export.so"
    src = [os.path.join(ROOT, "tests", "native", "bvh_check.cpp"), os.path.join(ROOT, "beifong_amd", "csrc", "bf_bvh.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread"] + flags + ["-o", str(out)] + src, check=True)
    lib = C.CDLL(str(out))
    lib.bvh_export.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32 * 4)]
    return lib


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return _build(tmp_path_factory, "sah16", [])


@pytest.fixture(scope="module")
def host8(tmp_path_factory):
    return _build(tmp_path_factory, "sah8", ["-DBF_SAH_BINS=8"])


def export(lib, v, f):
    """(nodes4, nodes16, rows, root4, root16, origin scale) of the host builder's trees, in read_bvh's form: the rows in leaf order
    with the input triangle's index as the primitive word"""
    tri = np.ascontiguousarray(np.asarray(v, f32)[np.asarray(f)].reshape(-1, 9))
    n = tri.shape[0]
    order = np.zeros(n, np.uint32)
    n4, n16 = np.zeros(n + 1, capi.NODE4_DTYPE), np.zeros(n + 1, capi.NODE16_DTYPE)
    out = (C.c_uint32 * 4)()
    rc = lib.bvh_export(n, tri.ctypes.data, order.ctypes.data, n4.ctypes.data, len(n4), n16.ctypes.data, len(n16), C.byref(out))
    assert rc == 0, rc
    rows = np.zeros((n, 3, 4), f32)
    rows[:, :, :3] = tri.reshape(n, 3, 3)[order]
    rows.view(np.uint32)[:, 0, 3] = order
    roots = np.array([out[2], out[3]], np.uint32).view(np.int32)
    # build_bvh(tris, bvh, 0.f) pads for the largest |coordinate| of the soup
    return n4[:out[0]].copy(), n16[:out[1]].copy(), rows, int(roots[0]), int(roots[1]), f32(np.abs(tri).max())


def _verify(lib, name):
    n4, n16, rows, r4, r16, scale = export(lib, *mesh(name))
    check_tree(n4, rows, r4, 4)
    check_tree(n16, rows, r16, 16)
    rec = sah_ref.verify(n4, rows, r4, scale)
    assert sah_ref.check_wide(n16, r16, len(rows), rec) > 0
    for w, nodes in ((4, n4), (16, n16)):
        check_padding(nodes, rows, w, scale, "refit")          # the builder's own padding is the refit's rule (Builder::pad)
    return rec


@pytest.mark.parametrize("name", ["soup3000", "bus6000"])
def test_host_splits_are_the_sah_splits(host, name):
    rec = _verify(host, name)
    c = rec.counts
    assert c["forced"] == 0 and c["coincident"] == 0 and c["sah"] > len(mesh(name)[1]) // 4
    assert c["adoption_checked"] > 10 * max(1, c["adoption_skipped"])


@pytest.mark.parametrize("sizes", list(CLUSTERS), ids=lambda s: "-".join(map(str, s)))
def test_host_splits_between_clusters(host, sizes):
    rec = _verify(host, cluster_name(sizes))
    check_cluster_nodes(sizes, rec)


def test_host_forced_cuts(host):
    rec = _verify(host, "spiral")
    assert rec.counts["forced"] >= 1
    assert max(d for _, _, d in rec.nodes) <= 31


def test_host_coincident_cuts(host):
    rec = _verify(host, "copies")
    assert rec.counts["coincident"] >= 1


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 17])
def test_tiny_inputs(host, n):
    v, f = meshgen.triangle_soup(n, seed=n)
    n4, n16, rows, r4, r16, scale = export(host, v, f)
    rec = sah_ref.verify(n4, rows, r4, scale)
    sah_ref.check_wide(n16, r16, n, rec)
    assert (0, n, 0) in rec.nodes


# ---- the verifier can fail ---------------------------------------------------------------------------------------------------------
def test_eight_bins_are_rejected(host8):
    n4, n16, rows, r4, r16, scale = export(host8, *mesh("soup3000"))
    check_tree(n4, rows, r4, 4)                                # a valid tree all the same
    with pytest.raises(sah_ref.SplitRuleError, match="no grouping of its children follows the split rule"):
        sah_ref.verify(n4, rows, r4, scale)


def _rows_along_x(xs):
    """one small triangle per x"""
    rows = np.zeros((len(xs), 3, 4), f32)
    base = np.array([[0, 0, 0], [0.1, 0.02, 0.01], [0.03, 0.1, 0.05]], f32)
    for i, x in enumerate(xs):
        rows[i, :, :3] = base + np.array([x, 0, 0], f32)
    rows.view(np.uint32)[:, 0, 3] = np.arange(len(xs))
    return rows


def _node4(rows, children, scale):
    """one NODE4 record: children = [(reference, first, count)]"""
    node = np.zeros(1, capi.NODE4_DTYPE)
    for k in range(4):
        ref, lo, hi = EMPTY, np.full(3, np.inf, f32), np.full(3, -np.inf, f32)
        if k < len(children):
            ref, a, c = children[k]
            xyz = rows[a:a + c, :, :3].reshape(-1, 3)
            lo, hi = refit_pad(xyz.min(0), xyz.max(0), scale)
        for j, ax in enumerate("xyz"):
            node["lo" + ax][0, k], node["hi" + ax][0, k] = lo[j], hi[j]
        node["child"][0, k] = ref
    return node


def _leaf(first, count):
    return ~((first << 3) | (count - 1))


def test_a_wrong_grouping_is_rejected():
    scale = f32(12.0)
    good = _rows_along_x([0, 1, 10, 11])
    n4 = _node4(good, [(_leaf(0, 2), 0, 2), (_leaf(2, 2), 2, 2)], scale)
    check_tree(n4, good, 0, 4)
    rec = sah_ref.verify(n4, good, 0, scale)
    assert rec.counts["sah"] == 1 and (0, 4, 0) in rec.nodes and (2, 2, 1) in rec.nodes
    bad = _rows_along_x([0, 10, 1, 11])
    n4 = _node4(bad, [(_leaf(0, 2), 0, 2), (_leaf(2, 2), 2, 2)], scale)
    check_tree(n4, bad, 0, 4)                                  # valid, and every traversal returns the same hits
    with pytest.raises(sah_ref.SplitRuleError, match="the left set is no"):
        sah_ref.verify(n4, bad, 0, scale)


def test_a_three_child_node_with_an_internal_child_is_rejected():
    scale = f32(32.0)
    rows = _rows_along_x([0, 1, 10, 11, 20, 21, 30, 31])
    leaves = [(_leaf(2 * i, 2), 2 * i, 2) for i in range(4)]
    n4 = _node4(rows, leaves, scale)
    check_tree(n4, rows, 0, 4)
    rec = sah_ref.verify(n4, rows, 0, scale)                   # the collapse as the builders make it
    assert rec.counts["sah"] == 3 and rec.counts["adoption_checked"] == 1
    # the same binary tree with the right half left un-adopted
    n4 = np.concatenate([_node4(rows, [leaves[0], (1, 4, 4), leaves[1]], scale), _node4(rows, [leaves[2], leaves[3]], scale)])
    check_tree(n4, rows, 0, 4)
    with pytest.raises(sah_ref.SplitRuleError, match="adopts until it has four children or only leaves"):
        sah_ref.verify(n4, rows, 0, scale)
