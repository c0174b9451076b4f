"""Deform batches (bf_render_deform_batch_device): one geometry version per render, gathered from slice k of the
caller's vertex arrays, moved by to_world[k] and re-fitted for all renders at once.  Render k is held, path for path, to a vertex
update + a transform + a stand-alone render on a second handle, and one render to the oracle on the rebuilt description."""
import numpy as np
import pytest

from beifong_amd import capi, motion, scenes
from tests.hist_bound import assert_fp32_sum, count_channels
from tests.oracle_lib import OracleScene
from tests.rolling_helpers import _launch_like
from tests.test_gpu_deform import _has_normals, _target, _verts, deform
from tests.test_gpu_motion import _centre, _identity, _meshes, _multi_mesh, _receive_iq, _same

pytestmark = pytest.mark.gpu
f32 = np.float32
K = 8


def _frames(sd, k, n):
    """n frames of mesh k between its described vertices and the 'twist' deformation (and their normals)"""
    v0 = _verts(sd, k)
    v1, n1 = deform(sd, k, "twist")
    w = (0.5 - 0.5 * np.cos(np.pi * (np.arange(n) + 1) / n))[:, None, None]
    pos = np.ascontiguousarray((v0[None].astype(np.float64) * (1 - w) + v1[None].astype(np.float64) * w).astype(f32))
    nrm = None
    if _has_normals(sd, k):
        from beifong_amd import meshgen
        f = np.ctypeslib.as_array(sd.shapes[k].indices, shape=(sd.shapes[k].n_faces, 3))
        nrm = np.ascontiguousarray(np.stack([meshgen.vertex_normals(pos[i], f) for i in range(n)]).astype(f32))
    return pos, nrm


def _tables(sd, k, n):
    """another mesh than k turns and shifts rigidly, its own pose per render"""
    other = next(m for m in _meshes(sd) if m != k)
    xf = np.tile(_identity(sd)[None], (n, 1, 1, 1))
    for i in range(n):
        xf[i, other] = motion.about(motion.rotation([0, 0, 1], 11.0 * (i + 1)), _centre(sd, other), (0.05 * i, -0.03 * i, 0.0))
    return xf.astype(f32)


@pytest.mark.parametrize("own_seeds", [False, True], ids=["common_seed", "own_seeds"])
def test_batch_equals_update_transform_render(hiplib, own_seeds):
    sd, lp = _multi_mesh(True)
    k = _target(sd)
    pos, nrm = _frames(sd, k, K)
    xf = _tables(sd, k, K)
    seeds = [100 + i for i in range(K)] if own_seeds else None
    g = capi.Scene(sd)
    c = g.clone()
    _, r0, _ = g.render(lp, records=True)
    hb, rb, sb = g.render_deform_batch(lp, {k: pos}, normals={k: nrm}, transforms=xf, seeds=seeds, records=True)
    ref = capi.Scene(sd)
    for i in range(K):
        li = _launch_like(lp, seeds[i] if seeds else lp.seed, flags=lp.flags)
        ref.update_vertices(k, pos[i], nrm[i])
        ref.transform_meshes(xf[i])
        hs, rs, _ = ref.render(li, records=True)
        _same(rb[i], rs)
    # one render against the oracle on the rebuilt description
    i = 5
    li = _launch_like(lp, seeds[i] if seeds else lp.seed, flags=lp.flags)
    want = motion.moved_description(motion.deformed_description(sd, {k: (pos[i], nrm[i])}), xf[i])
    ho, ro, so, add = OracleScene(want).render(li, records=True, threads=8, addends=True)
    _same(rb[i], ro)
    assert_fp32_sum(hb[i], add.ref, add.S, add.N, f"deform batch render {i}", counts=count_channels(li, want))
    # the handle and its clone are as they were
    _same(g.render(lp, records=True)[1], r0)
    _same(c.render(lp, records=True)[1], r0)


def test_chunked_arena_and_no_transforms(hiplib, monkeypatch):
    """A small arena renders the batch in chunks (BF_MOTION_BATCH_MB, as the motion batch); to_world NULL; positions alone."""
    sd, lp = _multi_mesh(True)
    k = _target(sd)
    pos, _ = _frames(sd, k, K)
    seeds = [3, 1, 4, 1, 5, 9, 2, 6]
    _, rfull, sfull = capi.Scene(sd).render_deform_batch(lp, {k: pos}, seeds=seeds, records=True)
    g = capi.Scene(sd)
    # 1 MB: below one version of this scene, one render per chunk; 24 MB: a few versions per chunk, not all eight (one version
    # of these 30000 triangles with normals, both trees and the refit's scratch is several MB: tests/test_gpu_motion_batch.py)
    for mb in ("1", "24"):
        monkeypatch.setenv("BF_MOTION_BATCH_MB", mb)
        _, rch, sch = g.render_deform_batch(lp, {k: pos}, seeds=seeds, records=True)
        for i in range(K):
            _same(rch[i], rfull[i])
        assert sch.n_paths == sfull.n_paths == K * lp.n_paths and sch.n_guard == 0
        assert sch.n_bounce_iters > sfull.n_bounce_iters              # several launch sequences
    monkeypatch.delenv("BF_MOTION_BATCH_MB")
    ref = capi.Scene(sd)
    for i in (0, 3, 7):
        ref.update_vertices(k, pos[i])
        _same(rfull[i], ref.render(_launch_like(lp, seeds[i], flags=lp.flags), records=True)[1])


def test_batch_on_a_posed_and_updated_handle(hiplib):
    """the batch starts from the handle's BASE (its latest update), not from its pose; to_world is absolute"""
    sd, lp = _multi_mesh(False)
    k = _target(sd)
    other = next(m for m in _meshes(sd) if m != k)
    vo, _ = deform(sd, other, "ripple")
    pos, _ = _frames(sd, k, 3)
    xf = _tables(sd, k, 3)
    g = capi.Scene(sd)
    g.update_vertices(other, vo)
    g.transform_meshes(xf[2])
    _, rpose, _ = g.render(lp, records=True)
    _, rb, _ = g.render_deform_batch(lp, {k: pos}, transforms=xf, records=True)
    for i in range(3):
        want = motion.moved_description(motion.deformed_description(sd, {k: pos[i], other: vo}), xf[i])
        _same(rb[i], capi.Scene(want).render(lp, records=True)[1])
    _same(g.render(lp, records=True)[1], rpose)


def test_deform_sweep_equals_per_pulse(hiplib):
    pytest.importorskip("torch")
    from beifong_amd import sweep
    sd, lp = _receive_iq()
    k = _target(sd)
    pos, _ = _frames(sd, k, 6)
    xf = _tables(sd, k, 6) if len(_meshes(sd)) > 1 else None
    a = sweep.render_deform_sweep(sd, lp, {k: pos}, transforms=xf, n_streams=2)
    b = sweep.render_deform_sweep(sd, lp, {k: pos}, transforms=xf, n_streams=2, per_pulse=True)
    assert a.shape == b.shape and np.all(a[:, :, 2].sum(1) == b[:, :, 2].sum(1))
    # the same paths summed in another order: the fp32 summation bound of the per-pulse oracle
    i = 4
    want = motion.deformed_description(sd, {k: pos[i]})
    if xf is not None:
        want = motion.moved_description(want, xf[i])
    ho, ro, so, add = OracleScene(want).render(lp, records=True, threads=8, addends=True)
    for cube in (a, b):
        assert_fp32_sum(cube[i].reshape(-1), add.ref, add.S, add.N, f"sweep pulse {i}", counts=count_channels(lp, want))
