"""The traversal stack's overflow path (bf_device_core.h: LaneStack), run on purpose and held to the brute-force oracle.

A lane keeps its first 16 (wf_trace) or 32 (bf_render_kernel, the tail's traverse_quad, bf_trace_kernel) stack entries in LDS and the
rest in a per-thread HBM column sized from bf_scene_info.bvh_stack_need; the SPILL = true kernels are chosen when that need exceeds 32.
No mesh and no ray distribution elsewhere in the suite keeps more than a few entries alive (tests/test_deep_tree_host.py), so the
inputs here are made for it: tests/deep_tree.py's cones of plates and the rays from their apex.

Expected values come from the oracle with brute_force=True: traces t, prim, shape and uv bit for bit and any-hit equal, as
test_gpu_parity's _compare_trace; renders as its _render_compare_one (records and counters exact, every histogram cell within
tests/hist_bound.py's fp32 summation bound).  Before anything is compared every case reads the device's tree back and asserts, with the
CPU walker of tests/deep_tree.py, that the rays it feeds in go past the LDS part of the kernel the case is about; the walker supplies
no expected value.

Two kinds of deep rays.  An apex ray keeps stack_need entries alive and ends on the backstop, but that hit waits at the bottom of its
stack: a stack that lost its spilled rows would still answer it right (only a wild row index would show, as a fault).  A climbing ray
(tests/deep_tree.py: climbing_rays, render_scene(climb=...)) goes as deep and is answered by a plate next to the apex, through the
last entries pushed: the walker counts the rays whose answer changes when the entries from position 32 (or 16) on are lost, and
every case that compares results asserts that count too.

Measured on an MI355X, (n, r): stack_need / apex occupancy / climbing rays of 256 that need the entries from 32 on.  Host builder
(bf_scene_create): (120, 1.08) 31 / 31 / 0, (160, 1.06) 33 / 33 / 49, (960, 1.01) 42 / 42 / 137.  Device builder
(bf_scene_rebuild_bvh) on the (960, 1.01) cone: 42 / 42 / 137 (no longer cone was needed).  Primary rays of the "climb" sensor: 249 of
256 (228 and 245 in the two turned poses of the motion batch)."""
import functools

import numpy as np
import pytest

from beifong_amd import capi, motion
from tests import deep_tree as dt
from tests import fast_contract as fc
from tests.bvh_tree_check import check_scene
from tests.hist_bound import assert_fp32_sum, assert_two_fp32_sums, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _launch_like, _same_records
from tests.test_gpu_parity import _render_compare_one

pytestmark = pytest.mark.gpu
f32 = np.float32

BIG = (960, 1.01)
# (n, r): the range of bvh_stack_need the case is about (tests/test_deep_tree_host.py asserts the same of the host builder)
CONES = {(120, 1.08): (30, 32), (160, 1.06): (33, 35), BIG: (40, 93)}
N_APEX = 64
N_CLIMB = 256
N_RAYS = 4096


@functools.lru_cache(maxsize=None)
def _cone(n, r):
    return dt.cone_of_plates(n, r)


def _occupancy(g, rays, **kw):
    nodes, rows, root = g.read_bvh(4)
    return dt.stack_occupancy(nodes, rows, root, rays, **kw)


def _assert_deep(occ, depth, what):
    """at least half of the rays keep more than `depth` entries alive"""
    assert 2 * np.count_nonzero(occ > depth) >= len(occ), f"{what}: {np.count_nonzero(occ > depth)} of {len(occ)} rays above {depth}"


@functools.lru_cache(maxsize=None)
def _query_rays(cone):
    """(rays, index sets): 64 apex rays, 16 apex rays that end short of the backstop (deep misses), 16 reversed ones and the cone's
    256 climbing rays, padded with random rays to 4096.  The first 32 apex rays fill half of the first wave; everything else is
    shuffled, so spilling and non-spilling lanes share waves."""
    apex, short, rev, climb = dt.apex_rays(N_APEX), dt.apex_rays(16, maxt=1.0), dt.reversed_rays(16), dt.climbing_rays(*cone, N_CLIMB)
    rnd = np.concatenate([dt.random_rays(2000, 21), dt.random_rays(N_RAYS - N_APEX - 32 - N_CLIMB - 2000, 22, extent=0.5)])
    rest = np.concatenate([apex[32:], short, rev, climb, rnd])
    perm = np.random.default_rng(5).permutation(len(rest))
    rays = np.concatenate([apex[:32], rest[perm]])
    where = np.empty(len(rest), np.int64)
    where[perm] = np.arange(len(rest))           # rest[j] sits at rays[32 + where[j]]
    at = lambda a, b: 32 + where[a:b]
    idx = dict(apex=np.concatenate([np.arange(32), at(0, 32)]), short=at(32, 48), rev=at(48, 64), climb=at(64, 64 + N_CLIMB))
    rays.setflags(write=False)
    return rays, idx


def _needs(g, rays, k, **kw):
    nodes, rows, root = g.read_bvh(4)
    return dt.needs_entries_from(nodes, rows, root, rays, k, **kw)


@pytest.mark.parametrize("cone", list(CONES), ids=lambda c: f"n{c[0]}_r{c[1]}")
def test_queries(hiplib, cone):
    """trace_closest, trace_any and ray_intersect (bf_trace_kernel<SPILL>, 32 entries in LDS): the (120, 1.08) cone fills the
    non-spilling kernel to its brim, where push3 takes its conditional branch; the other two spill 1 and 10 rows."""
    from beifong_amd import scenes
    lo, hi = CONES[cone]
    sd = scenes.single_mesh(*_cone(*cone))
    g, o = capi.Scene(sd), OracleScene(sd, brute_force=True)
    rays, idx = _query_rays(cone)
    need = g.info().bvh_stack_need
    assert lo <= need <= hi, need
    occ, occ_any = _occupancy(g, rays), _occupancy(g, rays, any_hit=True)
    climb = rays[idx["climb"]]
    n32, n32_any = _needs(g, climb, 32), _needs(g, climb, 32, any_hit=True)
    print(f"queries cone {cone}: stack_need {need}, apex occupancy {occ[idx['apex']].min()} .. {occ[idx['apex']].max()}, "
          f"short {occ[idx['short']].max()}, reversed {occ[idx['rev']].max()}, climbing {occ[idx['climb']].min()} .. "
          f"{occ[idx['climb']].max()}, of which {n32.sum()} (closest) and {n32_any.sum()} (any) of {N_CLIMB} need entries from 32 on")
    assert occ.max() == need and occ_any.max() == need
    if need > 32:
        _assert_deep(occ[idx["apex"]], 32, "closest-hit apex rays")
        _assert_deep(occ_any[idx["apex"]], 32, "any-hit apex rays")
        _assert_deep(occ[idx["climb"]], 32, "climbing rays")
        # and the answers of at least half a wave of rays are read out of the spilled rows
        assert n32.sum() >= 32 and n32_any.sum() >= 32, (n32.sum(), n32_any.sum())
    else:
        # the brim: a node visit with more than 32 - 3 entries, where push3 leaves its unconditional writes
        _assert_deep(_occupancy(g, rays[idx["apex"]], at_visit=True), 29, "apex rays at the brim")
    # compare (test_gpu_parity: _compare_trace)
    tg, pg, sg, ug = g.trace_closest(rays)
    to, po, so, uo = o.trace_closest(rays)
    assert np.array_equal(tg.view(np.uint32), to.view(np.uint32))
    assert np.array_equal(pg, po) and np.array_equal(sg, so)
    hit = np.isfinite(to)
    assert np.array_equal(ug[hit].view(np.uint32), uo[hit].view(np.uint32))
    ag, ao = g.trace_any(rays), o.trace_any(rays)
    assert np.array_equal(ag, ao)
    # the hits carry the condition: every apex ray ends on the backstop, none of the short ones hits anything
    assert np.all(po[idx["apex"]] == 0) and np.all(to[idx["apex"]] > 1.3) and np.all(ao[idx["apex"]] == 1)
    assert not hit[idx["short"]].any() and not ao[idx["short"]].any()
    assert np.all(po[idx["rev"]] == 0)
    assert hit[idx["climb"]].all() and np.all(po[idx["climb"]] > cone[0] // 2)      # answered by plates next to the apex
    assert hit.sum() > N_APEX + 16 + N_CLIMB + 100           # the random rays hit too
    # ray_intersect: t, prim, shape of every ray; every field of the deep hits
    r = g.ray_intersect(rays)
    assert np.array_equal(r["t"].view(np.uint32), to.view(np.uint32))
    assert np.array_equal(r["prim"][hit], po[hit]) and np.array_equal(r["shape"][hit], so[hit])
    assert not r["raw"][~hit, 1:].any()
    for i in np.concatenate([idx["apex"], idx["rev"], idx["climb"][::8]]):
        ref = o.intersect_full(rays[i])
        for k in ("t", "p", "n", "sh_n", "sh_s", "sh_t", "wi", "prim_uv", "dp_du", "dp_dv"):
            a, b = np.atleast_1d(r[k][i]), np.atleast_1d(ref[k])
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (i, k, a, b)


# ---- renders of the (960, 1.01) cone -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _render_case(view="apex"):
    """(sd, lp, mesh shape, oracle output) of the cone scene; never modified.  view "apex": the sensor at the apex, every primary ray
    goes as deep as the tree allows and ends on the backstop; "climb": the sensor inside the corner, the primary rays are climbing rays
    whose hits are read out of the spilled rows (tests/deep_tree.py: render_scene)."""
    sd, lp, mesh = dt.render_scene(*_cone(*BIG), climb=BIG if view == "climb" else None)
    return sd, lp, mesh, OracleScene(sd, brute_force=True).render(lp, records=True, threads=8, addends=True)


def _flags(lp, flags):
    return _launch_like(lp, lp.seed, flags=lp.flags | flags)


def _primary_rays(g):
    return dt.sensor_rays(g.sensor_sample_ray(dt.film_grid(16)))


def _assert_primary_rays_spill(g, view="apex", what="", tree=None):
    """The primary rays keep more than 32 entries alive (at least half of them); under the "climb" view at least half of them also find
    their hit through the entries from 32 on, and (wf_trace) from 16 on.  Returns the figures."""
    need = g.info().bvh_stack_need
    assert need > 32, need
    nodes, rows, root = tree or g.read_bvh(4)
    rays = _primary_rays(g)
    occ = dt.stack_occupancy(nodes, rows, root, rays)
    _assert_deep(occ, 32, f"primary rays {what}")
    fig = dict(stack_need=need, occupancy=(int(occ.min()), int(occ.max())))
    if view == "climb":
        n32, n16 = dt.needs_entries_from(nodes, rows, root, rays, 32), dt.needs_entries_from(nodes, rows, root, rays, 16)
        fig.update(need_entries_from_32=int(n32.sum()), need_entries_from_16=int(n16.sum()), rays=len(rays))
        assert 2 * n32.sum() >= len(rays) and 2 * n16.sum() >= len(rays), (what, fig)
    return fig


ROUTES = ["default", "megakernel", "no_tail", "small_pool", "no_wide", "quant", "stats", "fast"]


@pytest.mark.parametrize("view", ["apex", "climb"])
def test_render_routes(hiplib, monkeypatch, view):
    """One launch (4096 paths, range mode) through every route a spilling traversal can take: wf_trace (16 entries in LDS) and the
    tail (default), bf_render_kernel<.., SPILL> alone (megakernel), wf_trace to the end (no tail), regenerated slots (small pool), the
    tail's traverse_quad<SPILL> on the four-wide tree (no sixteen-wide tree), node4q_decide's pushes (quantised nodes), the STATS
    forms, the fast-arithmetic build.  Every route against the brute-force oracle, and the routes pairwise."""
    sd, lp, _, oracle_out = _render_case(view)
    _, ro, so, add = oracle_out
    assert np.count_nonzero(ro["L"]) > lp.n_paths // 2          # the paths carry radiance
    hists = {}
    for route in ROUTES:
        with monkeypatch.context() as m:
            env = {"no_tail": ("BF_WF_TAIL", "0"), "small_pool": ("BF_WF_POOL", "1024"), "no_wide": ("BF_NO_WIDE_BVH", "1"),
                   "quant": ("BF_QUANT_BVH", "1")}.get(route)
            if env:
                m.setenv(*env)
            g = capi.Scene(sd)                                  # (after setenv: the tunables are read when the scene is created)
        figures = _assert_primary_rays_spill(g, view, route)
        if route == "quant":
            assert g.info().trace_node_bytes == 64
        l = _flags(lp, {"megakernel": capi.BF_FLAG_MEGAKERNEL, "stats": capi.BF_FLAG_STATS, "fast": capi.BF_FLAG_FAST}.get(route, 0))
        if route == "fast":
            h, st = _fast_route(g, sd, l, oracle_out)
        else:
            h, _, st = _render_compare_one(g, l, oracle_out, 2e-5)
            for other, ho in hists.items():
                assert_two_fp32_sums(h, ho, add.S, add.N, f"route {route} against {other}", counts=count_channels(lp, sd))
            hists[route] = h
        print(f"render {view} route {route}: {figures}, kernel_variant {st.kernel_variant:#x}, n_bounces_tail "
              f"{st.n_bounces_tail}, n_rays_tail {st.n_rays_tail}, n_rays_traced {st.n_rays_traced}, n_bounce_iters {st.n_bounce_iters}")
        assert st.n_guard == 0 and st.n_paths == lp.n_paths
        if route == "no_tail":
            assert st.n_bounces_tail == 0 and st.n_bounce_iters > 1 and st.n_rays_traced > 0
        if route == "no_wide":
            assert st.n_bounces_tail > 0
        if route == "stats":
            assert st.n_nodes_visited > 0 and st.n_tris_tested > 0
        g.close()
    assert len(hists) == len(ROUTES) - 1


def _fast_route(g, sd, l, oracle_out):
    """BF_FLAG_FAST (tests/fast_contract.py): the device histogram is the fp32 sum of the render's own records (a 1 x 1 box film), at
    most the contract's cap of 1 % of the paths disagree with the oracle's, and a fresh handle's one-kernel fast render gives the
    same records bit for bit (another kernel, another LDS depth, the same arithmetic)."""
    ho, ro, so, add = oracle_out
    assert fc.is_box_1x1(sd, l)
    h, r, st = g.render(l, records=True)
    assert st.kernel_variant & capi.BF_VARIANT_FAST
    agree, worst = fc.agreement(r, ro)
    print(f"fast route: {np.count_nonzero(~agree)} of {len(agree)} paths diverged, largest |dL| / |L| among the others {worst:.3g}")
    assert np.count_nonzero(~agree) <= 0.01 * len(agree)
    ref, S, N = fc.film_addends(r, l)
    assert_fp32_sum(h, ref, S, N, "fast route against its own records", counts=count_channels(l, sd))
    fresh = capi.Scene(sd)
    _, rm, sm = fresh.render(_flags(l, capi.BF_FLAG_MEGAKERNEL), records=True)
    _same_records(r, rm)
    assert sm.n_rays_closest == st.n_rays_closest and sm.n_rays_shadow == st.n_rays_shadow
    fresh.close()
    return h, st


def test_receive_render(hiplib):
    """The receive kernels' SPILL forms: a Wigner transmitter and receiver at the apex.  The receiver's rays leave over a cosine
    hemisphere about the axis; the cone's corner takes about a sixth of it (at least a tenth is asserted, of rays drawn from the same
    distribution), so spilling and shallow paths share every wave."""
    sd, lp = dt.receive_scene(*_cone(*BIG))
    oracle_out = OracleScene(sd, brute_force=True).render(lp, records=True, threads=8, addends=True)
    for flags in (0, capi.BF_FLAG_MEGAKERNEL):
        g = capi.Scene(sd)
        need = g.info().bvh_stack_need
        assert need > 32, need
        occ = _occupancy(g, dt.receiver_rays(2048, 3))
        assert np.count_nonzero(occ > 32) >= 0.10 * len(occ), np.count_nonzero(occ > 32)
        _, _, st = _render_compare_one(g, _flags(lp, flags), oracle_out, 2e-5)
        print(f"receive render flags {flags:#x}: stack_need {need}, {np.count_nonzero(occ > 32)} of {len(occ)} receiver rays above 32 "
              f"(max {occ.max()}), kernel_variant {st.kernel_variant:#x}, n_bounces_tail {st.n_bounces_tail}")
        assert st.n_guard == 0
        g.close()


def _cone_poses(sd, mesh):
    """three rigid poses of the cone that keep its apex at the sensor: the identity and two small turns about the apex"""
    apex = np.zeros(3)
    own = [motion.rigid(), motion.about(motion.rotation([0, 0, 1], 2.0), apex, (5e-7, 0.0, 0.0)),
           motion.about(motion.rotation([1, 1, 0], -1.5), apex, (0.0, 5e-7, -5e-7))]
    xf = np.tile(motion.rigid(), (len(own), len(sd.shapes), 1, 1)).astype(f32)
    for k, m in enumerate(own):
        xf[k, mesh] = m
    return xf


@pytest.mark.parametrize("flags", [0, capi.BF_FLAG_MEGAKERNEL], ids=["wavefront", "megakernel"])
@pytest.mark.parametrize("view", ["apex", "climb"])
def test_motion_batch(hiplib, view, flags):
    """Per-render geometry (kGeom) with SPILL: three poses of the cone in one batch, one topology and one block of spill columns.
    Every render against the oracle on motion.moved_description; its own geometry version is read back for the walker."""
    sd, lp, mesh, _ = _render_case(view)
    lp = _flags(lp, flags)
    xf = _cone_poses(sd, mesh)
    seeds = [31, 32, 33]
    g = capi.Scene(sd)
    root = g.read_bvh(4)[2]
    hb, rb, st = g.render_motion_batch(lp, xf, seeds=seeds, records=True)
    assert st.n_guard == 0 and st.n_paths == len(seeds) * lp.n_paths
    for k in range(len(seeds)):
        nodes, rows, _ = g.debug_read_tree(4, version=k)
        fig = _assert_primary_rays_spill(g, view, f"render {k}", tree=(nodes, rows, root))
        moved = motion.moved_description(sd, xf[k])
        _, ro, _, add = OracleScene(moved, brute_force=True).render(_launch_like(lp, seeds[k]), records=True, threads=8, addends=True)
        _same_records(rb[k], ro)
        assert_fp32_sum(hb[k], add.ref, add.S, add.N, f"motion batch render {k}", counts=count_channels(lp, moved))
        print(f"motion batch {view} flags {flags:#x} render {k}: {fig}, kernel_variant {st.kernel_variant:#x}, n_bounces_tail "
              f"{st.n_bounces_tail}")
    assert not np.array_equal(rb[0]["L"], rb[1]["L"])


def _trace_equals_oracle(g, o, rays):
    tg, pg, sg, ug = g.trace_closest(rays)
    to, po, so, uo = o.trace_closest(rays)
    assert np.array_equal(tg.view(np.uint32), to.view(np.uint32))
    assert np.array_equal(pg, po) and np.array_equal(sg, so)
    hit = np.isfinite(to)
    assert np.array_equal(ug[hit].view(np.uint32), uo[hit].view(np.uint32))
    assert np.array_equal(g.trace_any(rays), o.trace_any(rays))
    return hit


def test_growth_on_a_rebuild(hiplib):
    """A handle created shallow (960 triangles on a flat grid, stack_need <= 16) is deformed into the cone and rebuilt on the device:
    bf_scene_rebuild_bvh must grow the spill columns (bf_mesh.cpp: new_spill > old_spill), a clone taken afterwards gets columns of the
    new size, a clone taken before keeps the flat geometry and its own short columns.  Then back: cone -> flat -> rebuild; results
    stay right and the clone that still renders the cone keeps its columns.

    The device builder need not cut as the host's does; measured on an MI355X for the (960, 1.01) cone: stack_need 13 -> 42, apex and
    primary-ray occupancy 42, 137 of 256 climbing rays need the entries from 32 on (the host builder's figures: 42, 42, 137)."""
    v_cone, f = _cone(*BIG)
    v_flat, _ = dt.flat_plates(BIG[0])
    sd_flat, lp, mesh = dt.render_scene(v_flat, f)
    sd_cone = motion.deformed_description(sd_flat, {mesh: v_cone})
    o_flat, o_cone = OracleScene(sd_flat, brute_force=True), OracleScene(sd_cone, brute_force=True)
    out_flat = o_flat.render(lp, records=True, threads=8, addends=True)
    out_cone = o_cone.render(lp, records=True, threads=8, addends=True)
    rays, idx = _query_rays(BIG)

    g = capi.Scene(sd_flat)
    need0 = g.info().bvh_stack_need
    assert need0 <= 16, need0
    before = g.clone()
    g.update_vertices(mesh, v_cone)
    g.rebuild_bvh()
    need1 = g.info().bvh_stack_need
    check_scene(g)
    occ = _occupancy(g, rays[idx["apex"]])
    prim_occ = _occupancy(g, _primary_rays(g))
    n32 = _needs(g, rays[idx["climb"]], 32)
    print(f"growth: stack_need {need0} -> {need1} (device builder, cone {BIG}); apex occupancy {occ.min()} .. {occ.max()}, "
          f"primary rays {prim_occ.min()} .. {prim_occ.max()}, {n32.sum()} of {N_CLIMB} climbing rays need entries from 32 on")
    assert need1 > need0 and need1 > 32, (need0, need1)
    _assert_deep(occ, 32, "apex rays on the rebuilt tree")
    _assert_deep(prim_occ, 32, "primary rays on the rebuilt tree")
    assert n32.sum() >= 32, n32.sum()
    after = g.clone()
    assert after.info().bvh_stack_need == need1 and before.info().bvh_stack_need == need0
    for name, h in (("rebuilt handle", g), ("clone taken after", after)):
        hit = _trace_equals_oracle(h, o_cone, rays)
        assert hit[idx["apex"]].all() and hit[idx["climb"]].all() and not hit[idx["short"]].any(), name
        _render_compare_one(h, lp, out_cone, 2e-5)
        _render_compare_one(h, _flags(lp, capi.BF_FLAG_MEGAKERNEL), out_cone, 2e-5)
    flat_rays = np.concatenate([dt.apex_rays(N_APEX), dt.random_rays(2000, 23)])
    assert _trace_equals_oracle(before, o_flat, flat_rays)[:N_APEX].any()
    _render_compare_one(before, lp, out_flat, 2e-5)
    # and back: the handle is shallow again, the clone taken in between still walks the cone with the columns it owns
    g.update_vertices(mesh, v_flat)
    g.rebuild_bvh()
    need2 = g.info().bvh_stack_need
    check_scene(g)
    assert need2 <= 16 and after.info().bvh_stack_need == need1, (need2, need1)
    _trace_equals_oracle(g, o_flat, flat_rays)
    _render_compare_one(g, lp, out_flat, 2e-5)
    _trace_equals_oracle(after, o_cone, rays)
    _render_compare_one(after, lp, out_cone, 2e-5)
    late = g.clone()
    _render_compare_one(late, lp, out_flat, 2e-5)
    # once more up, on a handle whose columns were sized for the cone before
    g.update_vertices(mesh, v_cone)
    g.rebuild_bvh()
    assert g.info().bvh_stack_need == need1
    _trace_equals_oracle(g, o_cone, rays)
    _render_compare_one(g, lp, out_cone, 2e-5)
    _render_compare_one(late, lp, out_flat, 2e-5)
    for h in (g, before, after, late):
        h.sync()


def test_two_handles_on_two_streams(hiplib):
    """test_gpu_parity's test_concurrent_renders_on_two_streams on the cone: two handles render side by side, each into the spill
    columns it owns; every render equals the oracle's."""
    torch = pytest.importorskip("torch")
    sd, lp, _, (ho, ro, so, add) = _render_case()
    handles = [capi.Scene(sd), capi.Scene(sd)]
    for g in handles:
        _assert_primary_rays_spill(g)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    nch = handles[0].channels(lp)
    hists = [torch.zeros(nch, device="cuda") for _ in range(6)]
    recs = [torch.zeros((int(lp.n_paths), 4), dtype=torch.int32, device="cuda") for _ in range(6)]
    for k, (h, r) in enumerate(zip(hists, recs)):
        j = k & 1
        with torch.cuda.stream(streams[j]):
            h.zero_()
            handles[j].render_device(lp, h.data_ptr(), stream=streams[j].cuda_stream, records_ptr=r.data_ptr())
    torch.cuda.synchronize()
    for k, (h, r) in enumerate(zip(hists, recs)):
        rec = np.ascontiguousarray(r.cpu().numpy()).view(np.uint32).view(capi.PATH_RECORD_DTYPE).reshape(-1)
        _same_records(rec, ro)
        assert_fp32_sum(h.cpu().numpy(), add.ref, add.S, add.N, f"stream render {k}", counts=count_channels(lp, sd))
    for g in handles:
        g.sync()
