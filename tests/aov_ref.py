"""Expected cells of a BF_FLAG_AOV render, built from what the oracle exports without knowing about AOVs.

Per pixel the render writes  X Y Z A W | the table's K floats | nested AOVs | nested.R G B A  (beifong_hip.h, at the flag).

    values   the SurfaceInteraction of every path's first ray: the ray composed as class_ref.first_hits composes it
             (bfo_sampler_floats -> sensor_sample_ray; with a crop window x = ((pixel + crop + fx) - crop) / W in float32, as
             generate_path writes it), OracleScene.intersect_full on it; zeros on a miss.  uv is prim_uv, or for a mesh with
             texture coordinates (uv0 * b0 + uv1 * b1) + uv2 * b2 in numpy float32, b0 = (1 - b1) - b2, from the
             description's texcoords.  duv_dx / duv_dy are zeros.
    weights  every path rendered alone by the oracle (class_ref.single_path_hists): its W channel is non-zero in exactly the
             pixels the sample lands in and holds the filter weight w there (1 under the box filter), exactly: one addend.
             A path whose single render adds nothing was dropped or cropped and adds nothing here.
    addend   float32(w) * float32(x), accumulated per cell as ref, S = sum |a| and N = non-zero addends in float64.

Base channels and the nested AOV block are the oracle's Addends of the plain launch, moved to their channels.  nested.A takes
w * valid.  nested.R = G = B takes w * record.L where the sensor's ray weight is 1 (perspective), as moment_ref does for
nested.XYZ; elsewhere those three channels are not checked (Expected.checked).

Self-checks: the composed hit equals record.valid for every path; composed t < far_clip for perspective sensors; the W cells of
the single renders add up to the plain launch's W channel (N exactly).
"""
import ctypes as C

import numpy as np

from beifong_amd import capi
from tests import oracle_lib
from tests.class_ref import single_path_hists
from tests.hist_bound import assert_fp32_sum, assert_two_fp32_sums
from tests.moment_ref import copy_launch
from tests.oracle_lib import OracleScene

ALL_NINE = list(range(capi.BF_AOV_TYPES))      # K = 22: 1 + 3 + 2 + 3 + 3 + 3 + 3 + 2 + 2


def with_aov(lp, extra=0):
    return copy_launch(lp, flags=lp.flags | capi.BF_FLAG_AOV | extra)


def plain_of(lp):
    return copy_launch(lp, flags=lp.flags & ~capi.BF_FLAG_AOV)


def _wide(sd):
    return np.float32(sd.desc.sensor.rfilter.radius) > np.float32(0.5) + np.float32(1500 * 2.0 ** -24)


def _shapes(sd):
    """the shapes of a SceneDesc, or of the holder a host scene's flat_desc returns (its .desc alone)"""
    return sd.shapes if hasattr(sd, "shapes") else [sd.desc.shapes[i] for i in range(sd.desc.n_shapes)]


def _sensor(sd):
    return sd.sensor if hasattr(sd, "sensor") else sd.desc.sensor


def first_rays(sd, lp):
    """the first ray of every path of `lp` on `sd`, [n, 8] float32 (o, mint, d, inf)"""
    lib = oracle_lib.load()
    n = int(lp.n_paths)
    compose = OracleScene(sd)
    sensor = _sensor(sd)
    pinhole = sensor.type in (capi.BF_SENSOR_PERSPECTIVE, capi.BF_SENSOR_RADIANCEMETER)
    film = bool(lp.spp and lp.film_width and lp.film_height)
    W, H = (np.float32(lp.film_width), np.float32(lp.film_height)) if film else (np.float32(1), np.float32(1))
    cx, cy = (int(sensor.crop_offset_x), int(sensor.crop_offset_y)) if film else (0, 0)
    rays = np.zeros((n, 8), np.float32)
    u = np.zeros(4, np.float32)
    for p in range(n):
        lib.bfo_sampler_floats(C.c_uint64(lp.seed + lp.path_offset + p), 4, u.ctypes.data_as(C.c_void_p))
        fx, fy = np.float32(u[0]), np.float32(u[1])
        ax, ay = (0.5, 0.5) if pinhole else (float(u[2]), float(u[3]))
        x, y = fx, fy
        if film:
            q = (lp.path_offset + p) // lp.spp
            x = ((np.float32(q % lp.film_width + cx) + fx) - np.float32(cx)) / W
            y = ((np.float32(q // lp.film_width + cy) + fy) - np.float32(cy)) / H
        r = compose.sensor_sample_ray(float(x), float(y), ax, ay)
        rays[p, 0:3], rays[p, 3], rays[p, 4:7], rays[p, 7] = r["o"], r["mint"], r["d"], np.inf
    return rays


def _prim0(sd):
    """first primitive index of every shape: a rectangle is one primitive, a mesh one per face"""
    out, at = [], 0
    for s in _shapes(sd):
        out.append(at)
        at += int(s.n_faces) if s.type == capi.BF_SHAPE_MESH else 1
    return out


def _texcoord_uv(s, face, b1, b2):
    idx = np.ctypeslib.as_array(s.indices, shape=(3 * int(s.n_faces),))
    tc = np.ctypeslib.as_array(s.texcoords, shape=(int(s.n_vertices), 2)).astype(np.float32)
    i0, i1, i2 = (int(idx[3 * face + k]) for k in range(3))
    b1, b2 = np.float32(b1), np.float32(b2)
    b0 = np.float32(1) - b1 - b2
    return (tc[i0] * b0 + tc[i1] * b1) + tc[i2] * b2


def first_values(sd, lp, records):
    """[n, 7] lists per path: the values of the seven stored types (depth, position, uv, geo normal, shading normal, dp_du, dp_dv)
    as one float32 row of 18, zeros for a miss; and the hit mask"""
    rays = first_rays(sd, lp)
    osc = OracleScene(sd)
    t, prim, shape, _ = osc.trace_closest(rays)
    hit = np.isfinite(t)
    valid = records["valid"] != 0
    assert np.array_equal(hit, valid), f"composed first hit differs from record.valid for {int((hit != valid).sum())} of {len(hit)} paths"
    if _sensor(sd).type == capi.BF_SENSOR_PERSPECTIVE and hit.any():
        assert float(t[hit].max()) < float(_sensor(sd).far_clip), (float(t[hit].max()), float(_sensor(sd).far_clip))
    prim0, shapes = _prim0(sd), _shapes(sd)
    vals = np.zeros((len(hit), 18), np.float32)
    n_tex = 0
    for p in np.flatnonzero(hit):
        si = osc.intersect_full(rays[p])
        uv = np.array(si["prim_uv"], np.float32)
        s = shapes[int(shape[p])]
        if s.type == capi.BF_SHAPE_MESH and bool(s.texcoords):
            uv = _texcoord_uv(s, int(prim[p]) - prim0[int(shape[p])], uv[0], uv[1])
            n_tex += 1
        vals[p] = np.concatenate([[si["t"]], si["p"], uv, si["n"], si["sh_n"], si["dp_du"], si["dp_dv"]]).astype(np.float32)
    return vals, hit, n_tex


_OFF = (0, 1, 4, 6, 9, 12, 15, 18)      # where each stored type starts in a row of first_values


def entry_values(vals, ty):
    """[n, floats of the type] float32 of one table entry"""
    if ty >= 7:
        return np.zeros((vals.shape[0], 2), np.float32)
    return vals[:, _OFF[ty]:_OFF[ty + 1]]


class Expected(object):
    """ref, S, N of every cell ([pixels, chan_px]) of one AOV render; `counts`: the flat cells that are exact; `checked`: the flat
    cells that are held to anything (all of them where the sensor weight is 1)"""

    def __init__(self, ref, S, N, counts, checked, layout, vals, hit, n_tex):
        self.ref, self.S, self.N, self.counts, self.checked = ref, S, N, counts, checked
        self.layout, self.vals, self.hit, self.n_tex = layout, vals, hit, n_tex

    def _sel(self, a):
        return np.asarray(a).reshape(-1)[self.checked]

    def _counts(self):
        pos = np.full(self.ref.size, -1, np.int64)
        pos[self.checked] = np.arange(self.checked.size)
        return pos[self.counts]

    def check(self, hist, what):
        h = np.asarray(hist).reshape(-1)
        assert h.size == self.ref.size, (what, h.size, self.ref.size)
        return assert_fp32_sum(self._sel(h), self._sel(self.ref), self._sel(self.S), self._sel(self.N), what, counts=self._counts())

    def check_two(self, h1, h2, what):
        # (two device results are comparable in every cell whose S and N are known: the unchecked ones have none)
        return assert_two_fp32_sums(self._sel(h1), self._sel(h2), self._sel(self.S), self._sel(self.N), what, counts=self._counts())

    def plain_part(self, hist):
        """the base channels and nested AOVs of an AOV histogram in the plain launch's layout"""
        h = np.asarray(hist).reshape(-1, self.layout["chan_px"])
        return np.concatenate([h[:, :5], h[:, self.layout["nested"]]], axis=1).reshape(-1)


def expected(sd, lp, types, singles=None):
    """(Expected, oracle records, Addends of the plain launch) of launch `lp` (with or without the flag) with table `types`"""
    plain = plain_of(lp)
    types = [int(t) for t in capi.aov_types(types)]
    lay = capi.aov_layout(plain, types)
    _, rec, _, add = OracleScene(sd).render(plain, records=True, threads=8, addends=True)
    vals, hit, n_tex = first_values(sd, plain, rec)
    if singles is None:
        singles = single_path_hists(sd, plain)
    film = bool(plain.spp and plain.film_width and plain.film_height)
    pixels = plain.film_width * plain.film_height if film else 1
    C0, C1, K = add.ref.size // pixels, lay["chan_px"], lay["K"]
    ref, S, N = np.zeros((pixels, C1)), np.zeros((pixels, C1)), np.zeros((pixels, C1), np.int64)
    for dst, src in ((ref, add.ref), (S, add.S), (N, add.N.astype(np.int64))):
        src = src.reshape(pixels, C0)
        dst[:, :5] = src[:, :5]
        dst[:, lay["nested"]] = src[:, 5:]
    weight_one = _sensor(sd).type == capi.BF_SENSOR_PERSPECTIVE
    # one row of addend factors per path: the table's K floats, nested.R G B, nested.A
    x = np.zeros((int(plain.n_paths), K + 4), np.float32)
    for sl, ty in zip(lay["aovs"], types):
        x[:, sl.start - 5:sl.stop - 5] = entry_values(vals, ty)
    x[:, K:K + 3] = rec["L"][:, None]
    x[:, K + 3] = hit
    cols = np.concatenate([np.arange(5, 5 + K), np.arange(lay["nested_rgba"].start, lay["nested_rgba"].stop)])
    n_w = np.zeros(pixels, np.int64)
    for p in range(int(plain.n_paths)):
        nz, w = singles[p]
        sel = nz % C0 == 4
        for c, wv in zip(nz[sel] // C0, w[sel]):
            a = (np.float32(wv) * x[p]).astype(np.float64)      # the fp32 product
            ref[c, cols] += a
            S[c, cols] += np.abs(a)
            N[c, cols] += a != 0.0
            n_w[c] += 1
    assert np.array_equal(n_w, add.N.reshape(pixels, C0)[:, 4].astype(np.int64)), "the single renders' W cells are not the launch's"
    flat = lambda px_ch: (np.arange(pixels)[:, None] * C1 + np.asarray(px_ch)[None, :]).reshape(-1)
    counts = np.zeros(0, np.int64) if _wide(sd) else flat([3, 4, lay["nested_rgba"].stop - 1])
    unchecked = [] if weight_one else list(range(lay["nested_rgba"].start, lay["nested_rgba"].start + 3))
    checked = flat([c for c in range(C1) if c not in unchecked])
    return Expected(ref, S, N, counts, np.sort(checked), lay, vals, hit, n_tex), rec, add
