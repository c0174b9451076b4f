"""The statement of recomputed vertex normals (include/beifong_hip.h, BF_NORMALS_RECOMPUTE / bf_vertex_normals) in plain numpy:
every operation a float32 operation on float32 operands, the arc cosine the oracle's bfo_elementary(2, ...).  It shares no code
with the product: what bf_vertex_normals and the device kernel are held to, bit for bit.

    face f (p0, p1, p2):  n = cross(p1 - p0, p2 - p0), l2 = (nx^2 + ny^2) + nz^2; nothing unless l2 > 0; nh = n / sqrt(l2)
    corner j:             a = p[j+1] - p[j], b = p[j+2] - p[j]; la = sqrt(dot(a, a)), lb = sqrt(dot(b, b)); nothing unless
                          la > 0 and lb > 0; c = clamp(dot(a / la, b / lb), -1, 1); contribution nh * acos(c)
    vertex:               s = +0 plus its contributions in increasing face index; s / sqrt(dot(s, s)), or (1, 0, 0) if that is 0
"""
import numpy as np

from tests import oracle_lib

f32 = np.float32


def _dot(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _acos(c):
    c = np.ascontiguousarray(c, f32)
    out = np.empty_like(c)
    if c.size:
        oracle_lib.load().bfo_elementary(2, c.size, c.ctypes.data, out.ctypes.data)
    return out


def contributions(positions, faces):
    """float32[nf, 3, 3] (face, corner, component) and bool[nf, 3]: which corners contribute at all."""
    p = np.ascontiguousarray(positions, f32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    assert p.dtype == f32
    q = [p[f[:, k]] for k in range(3)]
    with np.errstate(all="ignore"):
        e1, e2 = q[1] - q[0], q[2] - q[0]
        n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1],
                      e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                      e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        l2 = _dot(n, n)
        face_ok = l2 > 0
        nh = n / np.sqrt(l2)[:, None]
        out = np.zeros((len(f), 3, 3), f32)
        ok = np.zeros((len(f), 3), bool)
        for j in range(3):
            a, b = q[(j + 1) % 3] - q[j], q[(j + 2) % 3] - q[j]
            la, lb = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b))
            ok[:, j] = face_ok & (la > 0) & (lb > 0)
            d = _dot(a / la[:, None], b / lb[:, None])
            c = np.where(d < -1, f32(-1), np.where(d > 1, f32(1), d)).astype(f32)
            c[~ok[:, j]] = 0                       # (not used; keeps NaN out of the oracle call)
            out[:, j] = nh * _acos(c)[:, None]
    assert n.dtype == f32 and out.dtype == f32
    return out, ok


def fan(n_faces=300, degenerate=False):
    """A cone-shaped open fan: vertex 0 is the apex of n_faces triangles (more than a block's 256 lanes), float32[n_faces + 2, 3]
    and uint32 faces.  degenerate=True appends, with EXACT zero area (two corners at one position, so both edge vectors of the
    cross product are equal):
      - vertex d at vertex 1's position, used by the good face (d, 3, 2) and by the zero-area face (0, 1, d): a zero-area face
        whose three vertices all belong to good faces too;
      - vertices e, e2 at vertex 2's position, named by the zero-area faces (e, e2, 3) and (e2, e, 5) alone: they get (1, 0, 0)."""
    t = np.linspace(0.0, 1.7 * np.pi, n_faces + 1)
    rim = np.stack([0.8 * np.cos(t) * (1.0 + 0.1 * np.sin(5 * t)), 0.8 * np.sin(t), 0.15 * np.cos(3 * t) - 0.3], -1)
    v = np.concatenate([[[0.0, 0.0, 0.2]], rim])
    f = [[0, i + 1, i + 2] for i in range(n_faces)]
    if degenerate:
        d = len(v)
        v = np.concatenate([v, v[1:2], v[2:3], v[2:3]])
        e, e2 = d + 1, d + 2
        f += [[0, 1, d], [d, 3, 2], [e, e2, 3], [e2, e, 5]]
    return np.ascontiguousarray(v, f32), np.asarray(f, np.uint32)


def normals_ref(positions, faces):
    """float32[nv, 3]: the statement, faces summed in the order given."""
    p = np.ascontiguousarray(positions, f32).reshape(-1, 3)
    f = np.asarray(faces).reshape(-1, 3).astype(np.int64)
    t, ok = contributions(p, f)
    s = np.zeros_like(p)
    for i in range(len(f)):                        # one float32 add per component and contribution, in face order
        for j in range(3):
            if ok[i, j]:
                s[f[i, j]] = s[f[i, j]] + t[i, j]
    with np.errstate(all="ignore"):
        ln = np.sqrt(_dot(s, s))
        out = s / ln[:, None]
    out[ln == 0] = (1.0, 0.0, 0.0)
    assert out.dtype == f32
    return out
