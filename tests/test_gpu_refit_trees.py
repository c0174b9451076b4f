"""What bf_scene_translate_meshes, bf_scene_transform_meshes, bf_scene_update_vertices[_device], the geometry versions of the motion
/ deform batches and every call after a bf_scene_rebuild_bvh WRITE on the device, read back through the library's
test hooks (bfdbg_scene_read_tree, bfdbg_scene_origin_scale) and held to tests/bvh_tree_check.py.

Renders cannot see a box that is a little too tight (the ray that would miss is one in billions) or too loose (no record changes),
so nothing here renders beyond the one short launch that shows the sticky guard clean.  Every comparison is one of
  - bit equality against a numpy float32 restatement of a documented rule (check_padding: refit_pad / bf_translate_kernel; the rows
    and vertex normals against motion.apply_rigid / motion.deformed_description of the description),
  - byte equality between two handles (history independence; a batch's geometry version against a handle posed the same way),
  - the float64 origin-scale bracket of bvh_tree_check.origin_scale_bounds,
plus check_scene's structure and check_quantised's containment, which are the contracts tests/test_bvh_host.py states.
tests/test_bvh_tree_check_host.py shows that each of these checks can fail."""
import functools

import numpy as np
import pytest

from beifong_amd import capi, meshgen, motion, scenes
from tests.bvh_tree_check import check_origin_scale, check_padding, check_quantised, check_scene, check_tree, origin_scale_bounds
from tests.rolling_helpers import _launch_like
from tests.test_gpu_deform import _target, deform
from tests.test_gpu_deform_batch import _frames, _tables
from tests.test_gpu_motion import _centre, _identity, _meshes, _multi_mesh, _poses, _receive_iq
from tests.test_gpu_rebuild import _clean

pytestmark = pytest.mark.gpu
f32 = np.float32
SCENES = ["mm_normals", "mm", "receive_iq", "soup1", "soup3", "soup17", "soup5000", "soup_small", "soup_far"]
CORE = ["mm_normals", "soup17"]          # the cases every knob runs
OFFSETS = [(0.3, -0.2, 0.05), (0.0, 300.0, 0.0), (-1e4, 0.0, 0.0), (0.0, 0.0, 0.0)]


@functools.lru_cache(maxsize=None)
def _scene(name):
    """(description, a short launch or None): descriptions are never modified, so one of each serves every test"""
    if name in ("mm_normals", "mm", "receive_iq"):
        sd, lp = _receive_iq() if name == "receive_iq" else _multi_mesh(name == "mm_normals")
        return sd, _launch_like(lp, lp.seed, flags=lp.flags, n_paths=4096)
    if name == "soup_small":
        v, f = meshgen.triangle_soup(300, seed=21)
        return scenes.single_mesh((v * f32(1e-3)).astype(f32), f), None          # the absolute term of the padding dominates
    if name == "soup_far":
        v, f = meshgen.triangle_soup(300, seed=22)
        return scenes.single_mesh((v + np.array([4000.0, -4000.0, 10.0], f32)).astype(f32), f), None      # the relative term does
    n = int(name[4:])
    v, f = meshgen.triangle_soup(n, seed=30 + n)
    return scenes.single_mesh(v, f), None


def _cases(names=SCENES):
    """(scene, knob) pairs: every scene with and without the quantised nodes, the core scenes also without the sixteen-wide tree"""
    return [(s, k) for s in names for k in ("default", "quant", "no_wide") if k != "no_wide" or s in CORE]


def _set_knob(monkeypatch, k):
    if k == "quant":
        monkeypatch.setenv("BF_QUANT_BVH", "1")
    elif k == "no_wide":
        monkeypatch.setenv("BF_NO_WIDE_BVH", "1")


def _read(g, version=-1):
    """{which: nodes} of the trees the handle has, the rows, the normals (or None)"""
    trees, rows, normals = {}, None, None
    for which in (4, 16, 64):
        try:
            nodes, rows, normals = g.debug_read_tree(which, version)
        except capi.BeifongError as e:
            if which == 4 or ("sixteen-wide" not in str(e) and "quantised" not in str(e)):
                raise
            continue
        trees[which] = nodes
    return trees, rows, normals


def _same_bytes(a, b, what):
    (ta, ra, na), (tb, rb, nb) = a, b
    assert ta.keys() == tb.keys()
    for w in ta:
        assert ta[w].tobytes() == tb[w].tobytes(), f"{what}: the {w} nodes differ"
    assert ra.tobytes() == rb.tobytes(), f"{what}: the rows differ"
    assert (na is None) == (nb is None) and (na is None or na.tobytes() == nb.tobytes()), f"{what}: the vertex normals differ"


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _expected(sd_want, rows):
    """(xyz [n, 3, 3], normals [n, 3, 3], has_normals [n], face [n], shape [n]) the rows must hold, from a description: slot t holds
    face (prim - first prim of its shape) of shape `shape`, its three vertices float for float"""
    w = rows.view(np.uint32)
    prim, shape = w[:, 0, 3].astype(np.int64), w[:, 1, 3].astype(np.int64)
    xyz, nrm = np.zeros((len(rows), 3, 3), f32), np.zeros((len(rows), 3, 3), f32)
    has, face = np.zeros(len(rows), bool), np.zeros(len(rows), np.int64)
    for k in np.unique(shape):
        s = sd_want.shapes[int(k)]
        m = shape == k
        p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3))
        ix = np.ctypeslib.as_array(s.indices, shape=(s.n_faces, 3))
        face[m] = prim[m] - prim[m].min()              # (every face of a mesh has a slot: the smallest is its first primitive)
        assert m.sum() == s.n_faces and np.array_equal(np.sort(face[m]), np.arange(s.n_faces))
        xyz[m] = p[ix[face[m]]]
        if s.normals:
            nrm[m] = np.ctypeslib.as_array(s.normals, shape=(s.n_vertices, 3))[ix[face[m]]]
            has[m] = True
    return xyz, nrm, has, face, shape


class _H:
    """A handle and what it has been told: enough to state the rows it must hold and to bracket its origin scale."""

    def __init__(self, sd, g=None, seen=()):
        self.sd, self.g = sd, g if g is not None else capi.Scene(sd)
        self.seen = list(seen)
        self.kind, self.pose, self.offset = 0, _identity(sd), np.zeros(3, f32)
        self.base = {}                   # {shape: (positions, normals or None)} of the vertex updates so far
        self.refit = False               # the boxes were last written by the refit (else: created, or shifted from the created ones)
        self.rebuilt_under_pose = False
        self._remember()
        self.keep = {}                   # slots a refused device update left at their base rows: {slot: (xyz, normals)}

    def _remember(self):
        trees, rows, _ = _read(self.g)
        self.created = {w: t for w, t in trees.items() if w != 64}, rows

    def clone(self):
        c = _H(self.sd, self.g.clone(), self.seen)
        c.kind, c.pose, c.offset, c.base, c.refit = self.kind, self.pose.copy(), self.offset.copy(), dict(self.base), self.refit
        return c

    def transform(self, xf):
        xf = np.asarray(xf, f32)
        self.g.transform_meshes(xf)
        self.seen.append(xf.copy())
        self.kind, self.pose, self.refit = 2, xf.copy(), True

    def _offset_table(self, off):
        xf = _identity(self.sd)
        for k in _meshes(self.sd):
            xf[k] = motion.rigid(t=off)
        return xf

    def translate(self, off):
        self.g.translate_meshes(off)
        self.kind, self.offset, self.pose = 1, np.asarray(off, f32), self._offset_table(off)
        if self.base or self.rebuilt_under_pose:      # through the refit: the pose over the updated base, every mesh counted
            self.seen.append({"xf": self.pose, "all": True})
            self.refit = True
        else:
            self.refit = False

    def update(self, k, v, n=None, device=None, bound=None, box=None):
        if device is None:
            self.g.update_vertices(k, v, n)
            box = (v.min(0), v.max(0))
        else:
            torch, stream = device
            dv = torch.from_numpy(np.ascontiguousarray(v)).cuda()
            dn = torch.from_numpy(np.ascontiguousarray(n)).cuda() if n is not None else None
            torch.cuda.synchronize()
            self.g.update_vertices_device(k, dv.data_ptr(), dn.data_ptr() if dn is not None else None, bound)
            self.hold = (dv, dn)
            box = ([-bound] * 3, [bound] * 3)        # the header: the device form pads for [-bound, bound]^3
        self.seen.append({"xf": self.pose, "all": True, "boxes": {k: box}})
        old = self.base.get(k, (None, None))
        self.base[k] = (v, n if n is not None else old[1])
        self.refit = True

    def rebuild(self):
        posed = self.kind != 0 or bool(self.base)
        self.g.rebuild_bvh()
        if posed:
            self.rebuilt_under_pose = True
        else:
            self._remember()

    def want_sd(self):
        """the description the handle's rows must equal: the updated base, then the pose (a translation leaves the normals alone)"""
        sd = motion.deformed_description(self.sd, {k: (v if n is None else (v, n)) for k, (v, n) in self.base.items()}) if self.base else self.sd
        return sd if self.kind != 2 else motion.moved_description(sd, self.pose)

    def verify(self, lp=None, skip_rows=False):
        g = self.g
        check_scene(g)
        S = g.debug_origin_scale()
        check_origin_scale(S, origin_scale_bounds(self.sd, self.seen))
        trees, rows, normals = _read(g)
        if g.info().n_bvh_nodes == 0:
            assert len(trees[4]) == 0
        rule = "refit" if self.refit else "translate"
        if self.kind != 0 or self.refit:
            for w in (4, 16):
                if w in trees:
                    before = (self.created[0][w], self.created[1]) if rule == "translate" else None
                    check_padding(trees[w], rows, w, S, rule, before=before, offset=self.offset)
        if 64 in trees:
            check_quantised(trees[64], trees[4])
        if not skip_rows:
            xyz, nrm, has, _, _ = _expected(self.want_sd(), rows)
            if self.kind == 1:
                xyz = xyz + self.offset                 # fl(v + d), every coordinate one float32 addition
            for t, (kx, kn) in self.keep.items():
                xyz[t], nrm[t] = kx, kn
            assert np.array_equal(_bits(rows[:, :, :3]), _bits(xyz)), "a row is not the description's vertex moved as documented"
            if normals is not None:
                assert np.array_equal(_bits(normals[:, :, :3][has]), _bits(nrm[has])), "a vertex normal is not the description's, turned as documented"
        _clean(g, lp)
        return S


def _turn(sd):
    xf = _identity(sd)
    for k in _meshes(sd):
        xf[k] = motion.about(motion.rotation([0, 0, 1], 180.0), _centre(sd, k))
    return xf


def _far(sd):
    xf = _identity(sd)
    xf[_meshes(sd)[0]] = motion.rigid(t=(2000.0, 0.0, 0.0))
    return xf


# ---- translate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", _cases())
def test_translate_on_a_fresh_handle(hiplib, monkeypatch, name, k):
    _set_knob(monkeypatch, k)
    sd, lp = _scene(name)
    h = _H(sd)
    h.verify(lp)                                         # the tree as created
    for off in OFFSETS:
        h.translate(off)
        h.verify(lp)
    if sd.shapes[_meshes(sd)[0]].n_faces == 1:
        assert h.g.info().n_bvh_nodes == 0


@pytest.mark.parametrize("name,k", _cases(CORE))
def test_translate_on_a_clone_and_after_other_calls(hiplib, monkeypatch, name, k):
    _set_knob(monkeypatch, k)
    sd, lp = _scene(name)
    parent = _H(sd)
    before = _read(parent.g)
    c = parent.clone()
    for off in OFFSETS[:3]:
        c.translate(off)
        c.verify(lp)
        _same_bytes(_read(parent.g), before, "the parent of a translated clone")
    # after a transform: a translation applies to the geometry as created
    h = _H(sd)
    h.transform(_poses(sd, 0))
    h.verify(lp)
    h.translate(OFFSETS[0])
    h.verify(lp)
    # after an update: through the refit
    t = _target(sd)
    v, n = deform(sd, t, "twist")
    u = _H(sd)
    u.update(t, v, n)
    u.verify(lp)
    for off in OFFSETS[:3]:
        u.translate(off)
        assert u.refit
        u.verify(lp)


# ---- transform ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", _cases())
def test_transform(hiplib, monkeypatch, name, k):
    _set_knob(monkeypatch, k)
    sd, lp = _scene(name)
    h = _H(sd)
    created = _read(h.g)
    for xf in (_poses(sd, 0), _poses(sd, 1), _poses(sd, 2), _turn(sd), _far(sd)):
        h.transform(xf)
        h.verify(lp)
    h.transform(_identity(sd))
    h.verify(lp)                                         # the boxes meet the refit's rule, and
    _, rows, normals = _read(h.g)
    assert rows.tobytes() == created[1].tobytes(), "the identity does not restore the rows as created bit for bit"
    assert normals is None or normals.tobytes() == created[2].tobytes(), "the identity does not restore the normals as created"
    if sd.shapes[_meshes(sd)[0]].n_faces == 1:
        assert h.g.info().n_bvh_nodes == 0


# ---- vertex updates -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("posed", [False, True], ids=["base", "posed"])
@pytest.mark.parametrize("name,k", _cases())
def test_update_vertices(hiplib, monkeypatch, name, k, posed):
    _set_knob(monkeypatch, k)
    sd, lp = _scene(name)
    t = _target(sd)
    h = _H(sd)
    if posed:
        h.transform(_poses(sd, 0))
    for kind in ("ripple", "twist", "mirror"):
        v, n = deform(sd, t, kind)
        h.update(t, v, n)
        h.verify(lp)
    if sd.shapes[t].n_faces == 1:
        assert h.g.info().n_bvh_nodes == 0


@pytest.mark.parametrize("posed", [False, True], ids=["base", "posed"])
@pytest.mark.parametrize("name,k", _cases(CORE + ["soup1", "soup_small"]))
def test_update_vertices_device(hiplib, monkeypatch, name, k, posed):
    torch = pytest.importorskip("torch")
    _set_knob(monkeypatch, k)
    sd, lp = _scene(name)
    t = _target(sd)
    h = _H(sd)
    if posed:
        h.transform(_poses(sd, 1))
    dev = (torch, None)
    for kind, slack in (("ripple", 1.0), ("twist", 3.0)):
        v, n = deform(sd, t, kind)
        h.update(t, v, n, device=dev, bound=slack * float(np.abs(v).max()))      # (a declared bound above the data: padded for it)
        h.g.sync()
        h.verify(lp)
    # one NaN vertex: the slots that use it keep their base rows (the previous update's), the call is reported once, the tree passes
    v2, n2 = deform(sd, t, "mirror")
    bad = v2.copy()
    bad[0, 1] = np.nan
    _, rows, _ = _read(h.g)
    ix = np.ctypeslib.as_array(sd.shapes[t].indices, shape=(sd.shapes[t].n_faces, 3))
    pxyz, pnrm, _, face, shape = _expected(h.want_sd(), rows)      # the rows as they stand, posed
    h.update(t, bad, n2, device=dev, bound=2.0 * float(np.abs(v2).max()))
    with pytest.raises(capi.BeifongError):
        h.g.sync()
    h.g.sync()
    touched = np.nonzero((shape == t) & (ix[np.where(shape == t, face, 0)] == 0).any(1))[0]
    assert touched.size
    h.keep = {int(s): (pxyz[s], pnrm[s]) for s in touched}
    h.base[t] = (np.nan_to_num(bad), h.base[t][1])          # (the NaN itself never reaches a row: its slots are the kept ones)
    h.verify(lp)


# ---- history independence -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", _cases(CORE))
def test_history_independence(hiplib, monkeypatch, name, k):
    _set_knob(monkeypatch, k)
    sd, lp = _scene(name)
    rng = np.random.default_rng(77)
    P = _poses(sd, 1)
    a, b = _H(sd), _H(sd)
    a.transform(_far(sd))
    for _ in range(40):                                  # inside the far pose: every mesh turned about its centre, shifted by metres
        xf = _identity(sd)
        for m in _meshes(sd):
            xf[m] = motion.about(motion.rotation(rng.normal(size=3), rng.uniform(0, 360)), _centre(sd, m), rng.uniform(-50, 50, 3))
        a.transform(xf)
    a.transform(P)
    b.transform(_far(sd))
    b.transform(P)
    _same_bytes(_read(a.g), _read(b.g), "42 poses against 2")
    assert a.g.debug_origin_scale() == b.g.debug_origin_scale()
    a.verify(lp)
    # three updates against the last one alone
    t = _target(sd)
    a, b = _H(sd), _H(sd)
    for kind in ("ripple", "mirror", "twist"):            # (the last one's box is the largest: one bound for both handles)
        a.update(t, *deform(sd, t, kind))
    b.update(t, *deform(sd, t, "twist"))
    assert a.g.debug_origin_scale() == b.g.debug_origin_scale(), "the three deformations do not share one bound: choose others"
    _same_bytes(_read(a.g), _read(b.g), "three updates against the last")
    a.verify(lp)
    # translate after translate
    a, b = _H(sd), _H(sd)
    for off in OFFSETS[:3]:
        a.translate(off)
    b.translate(OFFSETS[2])
    _same_bytes(_read(a.g), _read(b.g), "three translations against the last")
    assert a.g.debug_origin_scale() == b.g.debug_origin_scale()


# ---- after a rebuild ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,k", _cases(CORE + ["soup5000"]))
def test_calls_after_a_rebuild_under_a_pose(hiplib, monkeypatch, name, k):
    _set_knob(monkeypatch, k)
    sd, lp = _scene(name)
    t = _target(sd)
    h = _H(sd)
    h.transform(_poses(sd, 0))
    h.update(t, *deform(sd, t, "twist"))
    h.rebuild()
    check_scene(h.g)
    check_origin_scale(h.g.debug_origin_scale(), origin_scale_bounds(sd, h.seen))
    h.transform(_poses(sd, 2))
    h.verify(lp)
    h.update(t, *deform(sd, t, "ripple"))
    h.verify(lp)
    h.translate(OFFSETS[0])
    assert h.refit
    h.verify(lp)


# ---- geometry versions of the batches -------------------------------------------------------------------------------------------------
def _check_version(g, k, twin, S):
    ver = _read(g, k)
    _same_bytes(ver, _read(twin.g), f"geometry version {k} against a handle posed the same way")
    trees, rows, _ = ver
    check_tree(trees[4], rows, g.read_bvh(4)[2], 4, g.info())
    for w in (4, 16):
        if w in trees:
            if w == 16:
                check_tree(trees[16], rows, g.read_bvh(16)[2], 16)
            check_padding(trees[w], rows, w, S, "refit")
    if 64 in trees:
        check_quantised(trees[64], trees[4])


@pytest.mark.parametrize("k", ["default", "quant", "no_wide"])
def test_motion_batch_versions(hiplib, monkeypatch, k):
    _set_knob(monkeypatch, k)
    sd, lp = _scene("mm_normals")
    xfs = np.stack([_poses(sd, 0), _identity(sd), _poses(sd, 1)]).astype(f32)
    g = _H(sd)
    g.transform(_poses(sd, 2))                           # a pose of its own, which the batch must leave alone
    before, S0 = _read(g.g), g.g.debug_origin_scale()
    g.g.render_motion_batch(lp, xfs)
    twin = _H(sd)
    twin.transform(_poses(sd, 2))
    for xf in xfs:
        twin.transform(xf)
    for i in range(3):
        twin.transform(xfs[i])
        S = twin.verify()
        _check_version(g.g, i, twin, S)
    _same_bytes(_read(g.g), before, "the handle's own arrays after a motion batch")
    assert g.g.debug_origin_scale() == S0
    with pytest.raises(capi.BeifongError, match="status %d" % capi.BF_ERR_INVALID):
        g.g.debug_read_tree(4, 3)
    # chunked: the hook refuses, the render succeeds
    monkeypatch.setenv("BF_MOTION_BATCH_MB", "1")
    hist, _, _ = g.g.render_motion_batch(lp, xfs)
    monkeypatch.delenv("BF_MOTION_BATCH_MB")
    assert np.isfinite(hist).all() and hist.shape[0] == 3
    with pytest.raises(capi.BeifongError, match="status %d" % capi.BF_ERR_INVALID):
        g.g.debug_read_tree(4, 0)
    g.verify(lp)


@pytest.mark.parametrize("k", ["default", "quant", "no_wide"])
def test_deform_batch_versions(hiplib, monkeypatch, k):
    torch = pytest.importorskip("torch")
    _set_knob(monkeypatch, k)
    sd, lp = _scene("mm_normals")
    t = _target(sd)
    pos, nrm = _frames(sd, t, 3)
    xfs = _tables(sd, t, 3)
    bound = float(np.abs(pos).max())                     # what the host form declares to the device form
    g = _H(sd)
    before, S0 = _read(g.g), g.g.debug_origin_scale()
    g.g.render_deform_batch(lp, {t: pos}, normals={t: nrm}, transforms=xfs)
    twin = _H(sd)
    dev = (torch, None)
    for i in range(3):
        twin.update(t, pos[i], nrm[i], device=dev, bound=bound)
        twin.transform(xfs[i])
    for i in range(3):
        twin.update(t, pos[i], nrm[i], device=dev, bound=bound)
        twin.transform(xfs[i])
        twin.g.sync()
        S = twin.verify()
        _check_version(g.g, i, twin, S)
    _same_bytes(_read(g.g), before, "the handle's own arrays after a deform batch")
    assert g.g.debug_origin_scale() == S0
    monkeypatch.setenv("BF_MOTION_BATCH_MB", "1")
    hist, _, _ = g.g.render_deform_batch(lp, {t: pos}, normals={t: nrm}, transforms=xfs)
    monkeypatch.delenv("BF_MOTION_BATCH_MB")
    assert np.isfinite(hist).all() and hist.shape[0] == 3
    with pytest.raises(capi.BeifongError, match="status %d" % capi.BF_ERR_INVALID):
        g.g.debug_read_tree(4, 0)
    g.verify(lp)
