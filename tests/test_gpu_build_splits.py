"""The device BVH builder (bf_scene_rebuild_bvh, bf_build.hip) held to the split rule it shares with the host builder, and its collapse
kernels to the adoption rule: tests/sah_ref.py on the trees the rebuild left, read back with read_bvh.

tests/bvh_tree_check.py and tests/test_gpu_rebuild.py cannot see a builder that bins wrongly on one of its two paths, sweeps the wrong
prefix or miscounts a side: such a tree is valid and returns the same hits.  Here every binary node recovered from the four-wide tree
must be a forced cut, a coincident cut or a binned-SAH split whose cost is within (1 + 2e-6) of the least of the 45 candidates (the
margin is derived in tests/sah_ref.py), every collapse must have adopted the largest surface first, every sixteen-wide child must be
a node of the same binary tree, and every box must be, bit for bit, the union of its rows padded by the builder's rule.

Inputs: those of tests/test_sah_ref_host.py, and triangle soups of the sizes at which the builder changes path: kSmall = 64 (one wave
per node against one thread per triangle), the 256-position workgroups of bin_large_kernel (LDS histogram when a workgroup lies inside
one node, global bins when it is mixed; below 256 triangles no workgroup is uniform) and the 64-lane uniformity of bounds_large_kernel.
Where neither builder cut by count, the device tree must also be the host's: the same family of primitive sets under leaves and child
slots, and the same family of recovered binary nodes (the two builders differ only where bf_build.hip's header says: forced cuts, order
inside a leaf, node order).  No render and no full-size case."""
import numpy as np
import pytest

from beifong_amd import capi, meshgen, scenes
from tests import sah_ref
from tests.bvh_tree_check import check_padding, check_scene
from tests.test_gpu_deform import _target, deform
from tests.test_gpu_motion import _multi_mesh
from tests.test_sah_ref_host import CLUSTERS, check_cluster_nodes, cluster_name, mesh

pytestmark = pytest.mark.gpu

PATH_SIZES = (3, 4, 5, 64, 65, 66, 255, 256, 257, 513)
SHARED = ["soup3000", "bus6000"] + [cluster_name(s) for s in CLUSTERS]
BY_COUNT = ["spiral", "copies"]                     # inputs on which the builders cut by count (forced, coincident)


def _mesh(name):
    if name.startswith("soup_"):
        n = int(name[5:])
        return meshgen.triangle_soup(n, seed=40 + n)
    return mesh(name)


def _verify(g, what, padding):
    nodes, rows, root = g.read_bvh(4)
    scale = g.debug_origin_scale()
    rec = sah_ref.verify(nodes, rows, root, scale)
    wn, wrows, wroot = g.read_bvh(16)
    wide = sah_ref.check_wide(wn, wroot, len(rows), rec)
    print(f"{what}: {len(rows)} triangles, {len(nodes)} four-wide nodes, {len(rec.nodes)} binary nodes, {rec.counts}, "
          f"{wide} sixteen-wide child ranges")
    if padding:
        # the tree exactly as the rebuild left it: bf_mesh.cpp keeps the builder's own scale as the handle's
        check_padding(nodes, rows, 4, scale, "refit")
        check_padding(wn, wrows, 16, scale, "refit")
    return rec


@pytest.mark.parametrize("name", SHARED + BY_COUNT + [f"soup_{n}" for n in PATH_SIZES])
def test_rebuilt_splits_are_the_sah_splits(hiplib, name):
    v, f = _mesh(name)
    sd = scenes.single_mesh(v, f)
    g = capi.Scene(sd)
    g.rebuild_bvh()
    check_scene(g)
    dev = _verify(g, f"{name} device", True)
    host = _verify(capi.Scene(sd), f"{name} host", False)
    assert g.info().bvh_depth <= 31
    if name in BY_COUNT:
        kind = "forced" if name == "spiral" else "coincident"
        assert dev.counts[kind] >= 1 and host.counts[kind] >= 1
        return
    if name.startswith("clusters"):
        check_cluster_nodes([int(x) for x in name.split("_")[1:]], dev)
    # no cut by count on these inputs (the host builder's figures are those of tests/test_sah_ref_host.py; the device cuts by
    # count at the same depths and counts, so a cut by count here means another tree): the device tree is the host's
    for r in (dev, host):
        assert r.counts["forced"] == 0 and r.counts["coincident"] == 0, r.counts
    assert dev.counts["sah"] == host.counts["sah"]
    assert dev.slot_sets == host.slot_sets, "the primitive sets under leaves and child slots differ from the host builder's"
    assert dev.prim_sets == host.prim_sets, "the recovered binary nodes differ from the host builder's"


def test_multi_mesh_after_a_twist(hiplib):
    sd, _ = _multi_mesh(True)
    k = _target(sd)
    v, n = deform(sd, k, "twist")
    g = capi.Scene(sd)
    g.update_vertices(k, v, n)
    g.rebuild_bvh()
    rec = _verify(g, "multi-mesh twist device", False)
    assert rec.counts["sah"] > 0 and rec.counts["adoption_checked"] > 10 * max(1, rec.counts["adoption_skipped"])
