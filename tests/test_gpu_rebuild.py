"""bf_scene_rebuild_bvh: both trees rebuilt on the device, in place, over the geometry a handle renders now.

Closest hits do not depend on the accelerator, so every path after a rebuild is bit-identical to the one before it, hence to the
oracle on a description rebuilt from the same vertices — the yardstick of tests/test_gpu_deform.py and tests/test_gpu_motion.py,
whose helpers are used here.  Every rebuilt tree is also walked by tests/bvh_tree_check.py, which the host builder's tree of a
freshly created scene must pass too.

Tolerances: none of its own.  Exact mode: records bit for bit, histogram cells within tests/hist_bound.py's fp32 summation bound
of the oracle; BF_FLAG_FAST: equal records and ray counts against a freshly created GPU scene.

The allocation-failure path is tested through the library's test hook (bfdbg_rebuild_fail_alloc)."""
import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, scenes
from tests.bvh_tree_check import check_scene, check_tree, prim_shape_multiset
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _Sequence, _launch_like
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.test_gpu_deform import _oracle_check, _target, _verts, deform
from tests.test_gpu_deform_batch import _frames, _tables
from tests.test_gpu_motion import _identity, _meshes, _multi_mesh, _poses, _rays_at, _receive_iq, _same, _with_flags
from tests.test_gpu_parity import _rays

pytestmark = pytest.mark.gpu
f32 = np.float32


def _clean(g, lp=None):
    """no device guard fired: bf_scene_sync raises if the sticky guard word is set (a ray dropped, a survivor claim refused), and
    a render with stats reports the same word as n_guard"""
    g.sync()
    if lp is not None:
        assert g.render(lp)[2].n_guard == 0
        g.sync()


def _bvh_bytes(g):
    out = []
    for w in (4, 16):
        try:
            nodes, rows, root = g.read_bvh(w)
        except RuntimeError as e:
            assert "sixteen-wide" in str(e)
            continue
        out.append((nodes.tobytes(), rows.tobytes(), root))
    return out


def test_host_tree_passes_the_checker(hiplib):
    """the checker is not stricter than the contract: bf_scene_create's own trees pass it"""
    for sd, _ in (_multi_mesh(True), _receive_iq()):
        check_scene(capi.Scene(sd))
    v, f = meshgen.triangle_soup(5000, seed=3)
    check_scene(capi.Scene(scenes.single_mesh(v, f)))


@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("kind", ["ripple", "twist", "mirror"])
@pytest.mark.parametrize("case", ["range", "range_normals", "receive_iq"])
def test_parity_after_a_deformation(hiplib, case, kind, fast):
    sd, lp = _receive_iq() if case == "receive_iq" else _multi_mesh(case == "range_normals")
    lp = _with_flags(lp, capi.BF_FLAG_FAST if fast else 0)
    k = _target(sd)
    v, n = deform(sd, k, kind)
    g = capi.Scene(sd)
    before = check_scene(g)
    g.update_vertices(k, v, n)
    _, r1, s1 = g.render(lp, records=True)
    g.rebuild_bvh()
    h2, r2, s2 = g.render(lp, records=True)
    _same(r2, r1)
    assert s2.n_rays_closest == s1.n_rays_closest and s2.n_rays_shadow == s1.n_rays_shadow
    check_scene(g, before)
    fresh_sd = motion.deformed_description(sd, {k: (v, n)})
    if fast:
        _, rf, sf = capi.Scene(fresh_sd).render(lp, records=True)
        _same(r2, rf)
        assert s2.n_rays_closest == sf.n_rays_closest and s2.n_rays_shadow == sf.n_rays_shadow
    else:
        _oracle_check(fresh_sd, lp, h2, r2, f"rebuild {case} {kind}")
    _clean(g, lp)


def test_noop_rebuild(hiplib):
    sd, lp = _multi_mesh(True)
    g = capi.Scene(sd)
    rays = _rays_at(sd, _identity(sd), 4000, 7)
    a = g.ray_intersect(rays)
    _, r0, _ = g.render(lp, records=True)
    before = check_scene(g)
    g.rebuild_bvh()
    check_scene(g, before)
    b = g.ray_intersect(rays)
    for key in a:
        x, y = np.asarray(a[key]), np.asarray(b[key])
        assert np.array_equal(x.view(np.uint32) if x.dtype == np.float32 else x, y.view(np.uint32) if y.dtype == np.float32 else y), key
    _same(g.render(lp, records=True)[1], r0)
    _clean(g)
    # a soup against the oracle's brute-force scene
    v, f = meshgen.triangle_soup(20000, seed=11)
    ssd = scenes.single_mesh(v, f)
    s = capi.Scene(ssd)
    s.rebuild_bvh()
    check_scene(s)
    o = OracleScene(ssd, brute_force=True)
    rays = _rays(20000, 111)
    tg, pg, sg, ug = s.trace_closest(rays)
    to, po, so, uo = o.trace_closest(rays)
    assert np.array_equal(tg.view(np.uint32), to.view(np.uint32)) and np.array_equal(pg, po) and np.array_equal(sg, so)
    hit = np.isfinite(to)
    assert hit.sum() > 1000 and np.array_equal(ug[hit].view(np.uint32), uo[hit].view(np.uint32))
    assert np.array_equal(s.trace_any(rays), o.trace_any(rays))


def test_composition_with_the_pose(hiplib):
    sd, lp = _multi_mesh(True)
    k = _target(sd)
    v, n = deform(sd, k, "twist")
    xf, xf2 = _poses(sd), _poses(sd, 1)
    # rebuild, then transform: the oracle on the moved description
    a = capi.Scene(sd)
    a.rebuild_bvh()
    a.transform_meshes(xf)
    ha, ra, _ = a.render(lp, records=True)
    _oracle_check(motion.moved_description(sd, xf), lp, ha, ra, "rebuild, transform")
    # transform, rebuild, update, transform again == create-with-V + transform (the pose stays absolute from the base)
    b = capi.Scene(sd)
    b.transform_meshes(xf)
    b.rebuild_bvh()
    check_scene(b)
    _same(b.render(lp, records=True)[1], ra)
    b.update_vertices(k, v, n)
    b.transform_meshes(xf2)
    hb, rb, _ = b.render(lp, records=True)
    new_sd = motion.deformed_description(sd, {k: (v, n)})
    _oracle_check(motion.moved_description(new_sd, xf2), lp, hb, rb, "transform, rebuild, update, transform")
    b.rebuild_bvh()
    check_scene(b)
    _same(b.render(lp, records=True)[1], rb)
    # a translation after a rebuild under a pose
    off = [0.3, -0.2, 0.05]
    b.translate_meshes(off)
    ref = capi.Scene(new_sd)
    ref.translate_meshes(off)
    _same(b.render(lp, records=True)[1], ref.render(lp, records=True)[1])
    # batches issued after a rebuild equal the stand-alone renders
    c = capi.Scene(sd)
    c.update_vertices(k, v, n)
    c.rebuild_bvh()
    table = np.stack([xf, xf2, _identity(sd)])
    seeds = [5, 6, 7]
    _, rm, _ = c.render_motion_batch(lp, table, seeds=seeds, records=True)
    for i, seed in enumerate(seeds):
        one = capi.Scene(motion.moved_description(new_sd, table[i]))
        _same(rm[i], one.render(_launch_like(lp, seed, flags=lp.flags), records=True)[1])
    v2, n2 = deform(sd, k, "ripple")
    pos = {k: np.stack([v, v2])}
    nrm = {k: np.stack([n, n2])} if n is not None else None
    _, rd, _ = c.render_deform_batch(lp, pos, nrm, seeds=[8, 9], records=True)
    for i, (vv, nn, seed) in enumerate(((v, n, 8), (v2, n2, 9))):
        one = capi.Scene(motion.deformed_description(sd, {k: (vv, nn)}))
        _same(rd[i], one.render(_launch_like(lp, seed, flags=lp.flags), records=True)[1])
    for g in (a, b, c):
        _clean(g)


def test_rolling_sequence_is_finished_by_the_rebuild(hiplib):
    pytest.importorskip("torch")
    sd, lp = _multi_mesh(False)
    g = capi.Scene(sd)
    seeds = [21, 22, 23, 24]
    seq = _Sequence(g, lp, seeds)
    seq.issue([0, 1])
    g.rebuild_bvh()                                           # finishes the open sequence
    h, recs = seq.results()
    ref = capi.Scene(sd)
    for i in (0, 1):
        hs, rs, ss = ref.render(_launch_like(lp, seeds[i]), records=True)
        _same(recs[i], rs)
        assert h[i][4] == hs[4] == lp.n_paths - ss.n_invalid  # complete histograms
    seq.issue([2, 3])
    g.flush()
    h, recs = seq.results()
    for i in (2, 3):
        l = _launch_like(lp, seeds[i])
        ho, ro, so, add = OracleScene(sd).render(l, records=True, threads=8, addends=True)
        _same(recs[i], ro)
        assert_fp32_sum(h[i], add.ref, add.S, add.N, f"rolling render {i} after the rebuild", counts=count_channels(l, sd))
    check_scene(g)
    _clean(g)


def test_clones(hiplib):
    sd, lp = _multi_mesh(True)
    g = capi.Scene(sd)
    c = g.clone()
    parent = _bvh_bytes(g)
    _, r0, _ = g.render(lp, records=True)
    c.rebuild_bvh()
    assert _bvh_bytes(g) == parent                            # copy on write: the parent's arrays are untouched
    assert _bvh_bytes(c) != parent
    _same(g.render(lp, records=True)[1], r0)
    _same(c.render(lp, records=True)[1], r0)
    c2 = c.clone()                                            # shares the rebuilt arrays
    assert _bvh_bytes(c2) == _bvh_bytes(c)
    _same(c2.render(lp, records=True)[1], r0)
    c.close()
    _same(c2.render(lp, records=True)[1], r0)
    # a deformed, posed handle and its clone
    k = _target(sd)
    v, n = deform(sd, k, "ripple")
    g.update_vertices(k, v, n)
    g.transform_meshes(_poses(sd))
    g.rebuild_bvh()
    _, r1, _ = g.render(lp, records=True)
    c3 = g.clone()
    _same(c3.render(lp, records=True)[1], r1)
    c3.rebuild_bvh()
    check_scene(c3)
    _same(c3.render(lp, records=True)[1], r1)
    for h in (g, c2, c3):
        _clean(h)


@pytest.mark.parametrize("knob", [{"BF_NO_WIDE_BVH": "1"}, {"BF_QUANT_BVH": "1"}], ids=["no_wide", "quant"])
def test_scene_options(hiplib, monkeypatch, knob):
    for key, val in knob.items():
        monkeypatch.setenv(key, val)
    for sd, lp in (_multi_mesh(True), _receive_iq()):
        k = _target(sd)
        v, n = deform(sd, k, "twist")
        g = capi.Scene(sd)
        if "BF_QUANT_BVH" in knob:
            assert g.info().trace_node_bytes == 64
        g.update_vertices(k, v, n)
        _, r1, _ = g.render(lp, records=True)
        g.rebuild_bvh()
        h2, r2, _ = g.render(lp, records=True)
        _same(r2, r1)
        fresh_sd = motion.deformed_description(sd, {k: (v, n)})
        _oracle_check(fresh_sd, lp, h2, r2, f"rebuild under {knob}")
        for flags in (0, capi.BF_FLAG_FAST):                  # fast mode: a freshly created GPU scene, as the deform tests do
            lf = _with_flags(lp, flags)
            _same(g.render(lf, records=True)[1], capi.Scene(fresh_sd).render(lf, records=True)[1])
        check_scene(g)
        if "BF_NO_WIDE_BVH" in knob:
            with pytest.raises(Exception, match="sixteen-wide"):
                g.read_bvh(16)
        # a transform re-fits (and re-quantises) the new topology
        g.transform_meshes(_poses(sd, 2))
        _, r3, _ = g.render(lp, records=True)
        _, rm, _ = capi.Scene(motion.moved_description(motion.deformed_description(sd, {k: (v, n)}), _poses(sd, 2))).render(lp, records=True)
        _same(r3, rm)
        _clean(g, lp)


def test_determinism(hiplib):
    sd, lp = _multi_mesh(True)
    k = _target(sd)
    v, n = deform(sd, k, "twist")
    g = capi.Scene(sd)
    g.update_vertices(k, v, n)
    g.rebuild_bvh()
    first = _bvh_bytes(g)
    g.rebuild_bvh()                                           # the rebuilt rows as input: a fixed point
    assert _bvh_bytes(g) == first
    h = capi.Scene(sd)                                        # the same geometry from the host builder's slot order
    h.update_vertices(k, v, n)
    h.rebuild_bvh()
    assert _bvh_bytes(h) == first


def _mesh_scene(v, f):
    return scenes.single_mesh(np.ascontiguousarray(v, f32), np.ascontiguousarray(f, np.uint32))


def test_degenerate_inputs(hiplib):
    rays = _rays(4000, 5)
    tri = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], f32)
    cases = {"one triangle": (tri, np.array([[0, 1, 2]], np.uint32)),
             "4096 copies": (tri, np.tile(np.array([[0, 1, 2]], np.uint32), (4096, 1)))}
    for name, (v, f) in cases.items():
        sd = _mesh_scene(v, f)
        g = capi.Scene(sd)
        t0 = g.trace_closest(rays)
        g.rebuild_bvh()
        check_scene(g)
        t1 = g.trace_closest(rays)
        for x, y in zip(t0, t1):
            assert np.array_equal(x.view(np.uint32) if x.dtype == f32 else x, y.view(np.uint32) if y.dtype == f32 else y), name
        assert g.info().bvh_depth <= 31, name
        _clean(g)
    # every vertex moved to one point, then onto a line
    v, f = meshgen.triangle_soup(3000, seed=2)
    sd = _mesh_scene(v, f)
    g = capi.Scene(sd)
    k = _meshes(sd)[0]
    nv = _verts(sd, k).shape[0]
    for name, q in (("point", np.tile(np.array([[0.25, -0.5, 0.125]], f32), (nv, 1))),
                    ("line", np.stack([np.linspace(-1, 1, nv), np.zeros(nv), np.full(nv, 0.5)], 1).astype(f32))):
        g.update_vertices(k, q)
        t0 = g.trace_closest(rays)
        g.rebuild_bvh()
        check_scene(g)
        t1 = g.trace_closest(rays)
        for x, y in zip(t0, t1):
            assert np.array_equal(x.view(np.uint32) if x.dtype == f32 else x, y.view(np.uint32) if y.dtype == f32 else y), name
        _clean(g)
    # rectangles only: nothing to do
    sd, lp = scenes.trans_rad(spp=64)
    g = capi.Scene(sd)
    _, r0, _ = g.render(lp, records=True)
    g.rebuild_bvh()
    _same(g.render(lp, records=True)[1], r0)
    assert g.info().n_bvh_nodes == 0
    _clean(g, lp)


@pytest.mark.parametrize("per_pulse", [False, True], ids=["batched", "per_pulse"])
def test_deform_sweep_with_rebuilds(hiplib, per_pulse):
    """render_deform_sweep(rebuild_every=2): the same paths as without rebuilds, every pulse within the oracle's summation bound"""
    pytest.importorskip("torch")
    from beifong_amd import sweep
    sd, lp = _receive_iq()
    k = _target(sd)
    pos, _ = _frames(sd, k, 6)
    xf = _tables(sd, k, 6) if len(_meshes(sd)) > 1 else None
    a = sweep.render_deform_sweep(sd, lp, {k: pos}, transforms=xf, n_streams=2, per_pulse=per_pulse, rebuild_every=2)
    b = sweep.render_deform_sweep(sd, lp, {k: pos}, transforms=xf, n_streams=2, per_pulse=per_pulse)
    assert a.shape == b.shape and np.all(a[:, :, 2].sum(1) == b[:, :, 2].sum(1))
    for i in (2, 5):                                          # pulses rendered after a rebuild
        want = motion.deformed_description(sd, {k: pos[i]})
        if xf is not None:
            want = motion.moved_description(want, xf[i])
        ho, ro, so, add = OracleScene(want).render(lp, records=True, threads=8, addends=True)
        assert_fp32_sum(a[i].reshape(-1), add.ref, add.S, add.N, f"sweep pulse {i}", counts=count_channels(lp, want))
    with pytest.raises(ValueError):
        sweep.render_deform_sweep(sd, lp, {k: pos}, rebuild_every=0)


def test_failure_leaves_the_scene_as_it_was(hiplib):
    sd, lp = _multi_mesh(True)
    k = _target(sd)
    v, n = deform(sd, k, "ripple")
    g = capi.Scene(sd)
    g.update_vertices(k, v, n)
    g.transform_meshes(_poses(sd))
    _, r0, _ = g.render(lp, records=True)
    before = _bvh_bytes(g)
    info0 = g.info()
    lib = g.lib
    try:
        for nth in (1, 5, 17, -1, -3, -6):
            lib.bfdbg_rebuild_fail_alloc(nth)
            with pytest.raises(Exception, match="bf_scene_rebuild_bvh"):
                g.rebuild_bvh()
            assert _bvh_bytes(g) == before, nth
            i = g.info()
            assert (i.n_bvh_nodes, i.bvh_depth, i.bvh_stack_need) == (info0.n_bvh_nodes, info0.bvh_depth, info0.bvh_stack_need)
    finally:
        lib.bfdbg_rebuild_fail_alloc(0)
    _same(g.render(lp, records=True)[1], r0)
    g.transform_meshes(_poses(sd, 1))                         # the pose and the refit state still work
    _, r1, _ = g.render(lp, records=True)
    new_sd = motion.deformed_description(sd, {k: (v, n)})
    _same(r1, capi.Scene(motion.moved_description(new_sd, _poses(sd, 1))).render(lp, records=True)[1])
    g.rebuild_bvh()
    _same(g.render(lp, records=True)[1], r1)
    _clean(g)


def test_full_size_c4(hiplib):
    """C4 (multi_mesh_radar, about 1.49 M triangles), the twist on the car, then the rebuild"""
    torch = pytest.importorskip("torch")
    sd, lp = scenes.multi_mesh_radar()
    k = max(_meshes(sd), key=lambda m: sd.shapes[m].n_faces)  # the car
    v, n = deform(sd, k, "twist")
    g = capi.Scene(sd)
    assert g.info().n_triangles > 1_400_000
    g.update_vertices(k, v, n)
    nr = 1 << 20
    # sensor rays: Sensor::sample_ray rows are o.xyz, mint, d.xyz, weight, maxt
    sr = g.sensor_sample_ray(np.random.default_rng(4).random((nr, 4)).astype(f32))
    rays = np.ascontiguousarray(np.concatenate([sr[:, 0:7], sr[:, 8:9]], 1), dtype=f32)
    d_rays = torch.from_numpy(rays).cuda()

    def shoot():
        si = torch.zeros((nr, capi.BF_SI_FLOATS), dtype=torch.float32, device="cuda")
        prim = torch.zeros(nr, dtype=torch.int32, device="cuda")
        shape = torch.zeros(nr, dtype=torch.int32, device="cuda")
        g.ray_intersect_device(nr, d_rays.data_ptr(), si.data_ptr(), prim.data_ptr(), shape.data_ptr())
        torch.cuda.synchronize()
        return si.cpu().numpy().view(np.uint32), prim.cpu().numpy(), shape.cpu().numpy()

    a = shoot()
    before = prim_shape_multiset(g.read_bvh(4)[1])
    g.rebuild_bvh()
    b = shoot()
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    check_scene(g, before)
    shard = _launch_like(lp, lp.seed, flags=lp.flags, n_paths=1 << 19)
    hg, rg, _ = g.render(shard, records=True)
    _oracle_check(motion.deformed_description(sd, {k: (v, n)}), shard, hg, rg, "C4 twist rebuilt")
    _clean(g)
