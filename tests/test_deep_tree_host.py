"""The inputs of tests/test_gpu_deep_tree.py measured on the CPU: the host builder's worst-case stack for the three cones of plates
(through bvh_check of tests/native/bvh_check.cpp), and how many entries their rays really keep alive (tests/deep_tree.py's walker
over bvh_export's tree).  Apex rays reach the builder's worst case exactly, so a spill column one row short would be written past;
random rays stay at or below 16 entries on the same trees (measured: 6, 8 and 13), which is why random-ray tests never run the
overflow path.  It also shows the walker's blind spot and its remedy: no apex ray's answer depends on the spilled entries, the
climbing rays' answers do.

The ranges asserted for stack_need are the contract of the GPU tests (which kernel forms each cone reaches); the exact values
measured with the current builder are 31, 33 and 42.  If a builder change moves a cone out of its range, choose a neighbouring r."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from beifong_amd import capi
from tests import deep_tree as dt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32

# (n, r): [lowest, highest] worst-case stack the GPU tests rely on
CONES = {(120, 1.08): (30, 32),       # the brim of the 32-entry kernels (push3's conditional branch); wf_trace spills
         (160, 1.06): (33, 35),       # the first spilled entries of the 32-entry kernels
         (960, 1.01): (40, 93)}       # ten rows and more


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    out = tmp_path_factory.mktemp("deep") / "libbvh_check.so"
    src = [os.path.join(ROOT, "tests", "native", "bvh_check.cpp"), os.path.join(ROOT, "beifong_amd", "csrc", "bf_bvh.cpp")]
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", str(out)] + src, check=True)
    lib = C.CDLL(str(out))
    lib.bvh_check.argtypes = [C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32 * 8)]
    lib.bvh_export.argtypes = [C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32 * 4)]
    return lib


def _host_tree(lib, v, f):
    """(statistics of bvh_check, (nodes4, rows, root4) of bvh_export in read_bvh's form)"""
    tri = np.ascontiguousarray(np.asarray(v, f32)[np.asarray(f)].reshape(-1, 9))
    n = tri.shape[0]
    out = (C.c_uint32 * 8)()
    rc = lib.bvh_check(n, tri.ctypes.data, C.byref(out))
    assert rc == 0, f"invariant {rc} violated"
    stats = dict(zip(("nodes4", "leaves", "max_leaf", "depth4", "stack_need", "depth2", "nodes2", "leaf_cap"), list(out)))
    order = np.zeros(n, np.uint32)
    n4, n16 = np.zeros(n + 1, capi.NODE4_DTYPE), np.zeros(n + 1, capi.NODE16_DTYPE)
    ex = (C.c_uint32 * 4)()
    rc = lib.bvh_export(n, tri.ctypes.data, order.ctypes.data, n4.ctypes.data, len(n4), n16.ctypes.data, len(n16), C.byref(ex))
    assert rc == 0, rc
    rows = np.zeros((n, 3, 4), f32)
    rows[:, :, :3] = tri.reshape(n, 3, 3)[order]
    root = int(np.array([ex[2]], np.uint32).view(np.int32)[0])
    return stats, (n4[:ex[0]].copy(), rows, root)


@pytest.mark.parametrize("cone", list(CONES), ids=lambda c: f"n{c[0]}_r{c[1]}")
def test_apex_rays_reach_the_builders_worst_case(lib, cone):
    lo, hi = CONES[cone]
    stats, tree = _host_tree(lib, *dt.cone_of_plates(*cone))
    print(f"cone {cone}: {stats}")
    assert lo <= stats["stack_need"] <= hi, stats
    assert stats["depth2"] <= 31 and stats["stack_need"] <= 3 * stats["depth4"], stats
    apex = dt.stack_occupancy(*tree, dt.apex_rays(32))
    print(f"cone {cone}: apex occupancy {apex.min()} .. {apex.max()}")
    assert apex.max() == stats["stack_need"]
    assert dt.stack_occupancy(*tree, dt.apex_rays(32), any_hit=True).max() == stats["stack_need"]
    # most of them, not one freak ray: what the GPU tests ask of the rays they feed in
    assert np.count_nonzero(apex > 16) >= 16
    if stats["stack_need"] > 32:
        assert np.count_nonzero(apex > 32) >= 16
    # every cone brings push3 of the 32-entry kernels to a node with more than 32 - 3 entries, where it leaves its unconditional writes
    assert np.count_nonzero(dt.stack_occupancy(*tree, dt.apex_rays(32), at_visit=True) > 29) >= 16
    # An apex ray goes deep, but its one hit waits at the bottom of its stack: losing the overflow part would not change its answer.
    # The climbing rays go as deep and are answered by the plates next to the apex, through the last entries pushed.
    assert not dt.needs_entries_from(*tree, dt.apex_rays(32), 16).any()
    climb = dt.climbing_rays(*cone)
    assert np.all(dt.stack_occupancy(*tree, climb) == stats["stack_need"])
    for any_hit in (False, True):
        n16, n32 = (int(dt.needs_entries_from(*tree, climb, k, any_hit=any_hit).sum()) for k in (16, 32))
        print(f"cone {cone}: {n16} / {n32} of {len(climb)} climbing rays need the entries from 16 / 32 on (any_hit={any_hit})")
        assert n16 >= len(climb) // 2
        assert n32 >= 32 if stats["stack_need"] > 32 else n32 == 0
    occ = dt.stack_occupancy(*tree, dt.random_rays(1000, 11))      # the distribution of test_gpu_parity's _rays
    assert occ.max() >= 1                                          # (they do enter the tree)
    print(f"cone {cone}: random-ray occupancy <= {occ.max()}")
    assert occ.max() <= 16
    # short of the backstop nothing is hit, and the descent is as deep
    short = dt.stack_occupancy(*tree, dt.apex_rays(32, maxt=1.0))
    assert short.max() >= stats["stack_need"] - 3, (short.max(), stats)


def test_flat_plates_are_shallow(lib):
    stats, tree = _host_tree(lib, *dt.flat_plates(960))
    assert stats["stack_need"] <= 16, stats
    assert dt.stack_occupancy(*tree, dt.apex_rays(32)).max() <= stats["stack_need"]


def test_the_scenes_start_their_paths_down_the_cone(lib):
    """The render scene's sensor sits at the apex: every primary ray (the oracle's sample_ray over a film grid with its corners) goes
    as deep as the tree allows and is answered by the backstop.  The receive scene's receiver sends a cosine hemisphere about the axis:
    the cone's corner takes about a sixth of it."""
    from tests.oracle_lib import OracleScene
    v, f = dt.cone_of_plates(960, 1.01)
    stats, tree = _host_tree(lib, v, f)
    sd, lp, mesh = dt.render_scene(v, f)
    o = OracleScene(sd, brute_force=True)
    rows = []
    for fx, fy, ax, ay in dt.film_grid(8):
        r = o.sensor_sample_ray(fx, fy, ax, ay)
        rows.append([*r["o"], r["mint"], *r["d"], r["weight"], np.inf])
    rays = dt.sensor_rays(np.array(rows, f32))
    assert np.all(dt.stack_occupancy(*tree, rays) == stats["stack_need"])
    t, prim, shape, _ = o.trace_closest(rays)
    assert np.all(prim == 0) and np.all(shape == mesh) and t.min() > 1.3
    # the sensor inside the corner: climbing rays, answered next to the apex out of the overflow part of a 32-entry stack
    sd, lp, mesh = dt.render_scene(v, f, climb=(960, 1.01))
    o = OracleScene(sd, brute_force=True)
    rows = []
    for fx, fy, ax, ay in dt.film_grid(8):
        r = o.sensor_sample_ray(fx, fy, ax, ay)
        rows.append([*r["o"], r["mint"], *r["d"], r["weight"], 100.0])
    rays = dt.sensor_rays(np.array(rows, f32))
    assert np.all(dt.stack_occupancy(*tree, rays) == stats["stack_need"])
    assert 2 * dt.needs_entries_from(*tree, rays, 32).sum() >= len(rays)
    t, prim, _, _ = o.trace_closest(rays)
    assert np.all(np.isfinite(t)) and prim.min() > 900
    occ = dt.stack_occupancy(*tree, dt.receiver_rays(2048, 3))
    print(f"receiver rays above 32 entries: {np.count_nonzero(occ > 32)} of {len(occ)}")
    assert np.count_nonzero(occ > 32) >= 0.10 * len(occ)


def _leaf(first, count):
    return ~((first << 3) | (count - 1))


def _hand_tree():
    """Root: the near child is node 1 (four leaves, the boxes x in [k, k + 0.5]), then three leaves at x in [4 + k, 4.5 + k].  Every box
    spans y, z in [0, 1]; triangle j is a plate in the plane x = its box's far side, covering y + z <= 1 of it."""
    nodes = np.zeros(2, capi.NODE4_DTYPE)
    xs = {1: [0.0, 1.0, 2.0, 3.0], 0: [0.0, 4.0, 5.0, 6.0]}
    for nd in (0, 1):
        for k, x in enumerate(xs[nd]):
            nodes[nd]["lox"][k], nodes[nd]["hix"][k] = x, x + 0.5
            nodes[nd]["loy"][k] = nodes[nd]["loz"][k] = 0.0
            nodes[nd]["hiy"][k] = nodes[nd]["hiz"][k] = 1.0
    nodes[0]["hix"][0] = 3.5                                # the internal child's box holds its four leaves
    nodes[1]["child"] = [_leaf(k, 1) for k in range(4)]
    nodes[0]["child"] = [1] + [_leaf(4 + k, 1) for k in range(3)]
    far = np.array([0.5, 1.5, 2.5, 3.5, 4.5, 5.5, 6.5], f32)
    rows = np.zeros((7, 3, 4), f32)
    rows[:, :, 0] = far[:, None]
    rows[:, 1, 1] = 1.0
    rows[:, 2, 2] = 1.0
    return nodes, rows, 0


def test_the_walker_counts_live_entries_on_a_hand_made_tree():
    tree = _hand_tree()
    ray = lambda o, d, maxt=np.inf: np.array([[*o, 1e-4, *d, maxt]], f32)
    occ = lambda r, **kw: int(dt.stack_occupancy(*tree, r, **kw)[0])
    # through the empty half (y + z > 1) of every box: three far children at the root, three more inside node 1
    assert occ(ray([-1, 0.8, 0.8], [1, 0, 0])) == 6
    assert occ(ray([-1, 0.8, 0.8], [1, 0, 0]), any_hit=True) == 6
    # the same line with the segment ending inside node 1's second box: two children there, node 1 alone at the root
    assert occ(ray([-1, 0.8, 0.8], [1, 0, 0], maxt=2.2)) == 1
    # through the plates: the closest-hit query meets the plate at x = 0.5 first and nothing behind it survives the narrowing; the far
    # children of the two node visits before that hit were pushed all the same
    assert occ(ray([-1, 0.2, 0.2], [1, 0, 0])) == 6
    # the other way round the nearest child of the root is its last leaf: two leaves and node 1 wait, and the hit at x = 6.5 ends it
    assert occ(ray([8, 0.2, 0.2], [-1, 0, 0])) == 3
    assert occ(ray([8, 0.8, 0.8], [-1, 0, 0])) == 3         # no hit: node 1 is entered last, when nothing else is left (3, not 5)
    # past everything, and a ray that touches one root leaf only
    assert occ(ray([-1, 2.0, 2.0], [1, 0, 0])) == 0
    assert occ(ray([5.2, 0.8, -1], [0, 0, 1])) == 0
    # several rays at once keep their own counts
    both = np.concatenate([ray([-1, 0.8, 0.8], [1, 0, 0]), ray([-1, 2.0, 2.0], [1, 0, 0]), ray([8, 0.2, 0.2], [-1, 0, 0])])
    assert dt.stack_occupancy(*tree, both).tolist() == [6, 0, 3]
    # an empty tree and a root that is one leaf
    assert dt.stack_occupancy(np.zeros(0, capi.NODE4_DTYPE), tree[1][:1], _leaf(0, 1), both).tolist() == [0, 0, 0]
