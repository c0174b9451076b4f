"""Per-mesh rigid motion (bf_scene_transform_meshes): the numpy statement of what the library does to a
mesh, and small helpers to build the 3x4 transforms it takes.

`apply_rigid` is the contract written out: a scene created from its outputs renders every path bit-identically to the
scene created from the original arrays and moved on the device.
"""
import math

import numpy as np

f32 = np.float32


def rotation(axis, deg):
    """float32[3, 3]: rotation by `deg` degrees about `axis` (right-handed; evaluated in float64, rounded once)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    ang = math.radians(float(deg))
    s, c = math.sin(ang), math.cos(ang)
    x, y, z = a
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]], dtype=np.float64).astype(f32)


def rigid(r=None, t=(0.0, 0.0, 0.0)):
    """float32[3, 4] = [R | t]; R defaults to the identity."""
    m = np.zeros((3, 4), f32)
    m[:, :3] = np.eye(3, dtype=f32) if r is None else np.asarray(r, dtype=f32).reshape(3, 3)
    m[:, 3] = np.asarray(t, dtype=f32).reshape(3)
    return m


def about(r, pivot, t=(0.0, 0.0, 0.0)):
    """float32[3, 4]: rotate by R about `pivot`, then translate by t (p' = R (p - pivot) + pivot + t, folded into [R | t'])."""
    r = np.asarray(r, dtype=np.float64).reshape(3, 3)
    pivot = np.asarray(pivot, dtype=np.float64).reshape(3)
    return rigid(r.astype(f32), (pivot - r @ pivot + np.asarray(t, dtype=np.float64)).astype(f32))


def twist(lin=(0.0, 0.0, 0.0), ang=(0.0, 0.0, 0.0), pivot=(0.0, 0.0, 0.0)):
    """float32[9] = [lin | ang | pivot], one bf_twist: the instantaneous rigid motion of a shape in world space.  A point p of it has
    velocity lin + ang x (p - pivot): lin in m/s, ang in rad/s, pivot in m.  A list of them, one per shape in scene-description
    order, is the `twists` of Scene.set_range_rate_classes; the default is a shape at rest."""
    return np.concatenate([np.asarray(v, dtype=f32).reshape(3) for v in (lin, ang, pivot)])


def vertex_velocities(p_prev, p_next, dt):
    """float32, the shape of p_prev: the world-space velocity of every vertex from its positions at two instants dt seconds apart,
    (p_next - p_prev) / dt in float32 with the difference and the quotient rounded on their own: a field for
    Scene.set_vertex_velocities (BF_VELOCITY_VERTEX), and what BF_VELOCITY_DIFFERENCE computes on the device from the rendered
    corners (capi.corner_velocities is the same arithmetic)."""
    a, b, t = np.asarray(p_prev, dtype=f32), np.asarray(p_next, dtype=f32), f32(dt)
    if not (np.isfinite(t) and t > 0):
        raise ValueError(f"dt must be finite and positive, got {dt}")
    with np.errstate(all="ignore"):
        return ((b - a) / t).astype(f32, copy=False)


def is_identity(m):
    m = np.asarray(m, dtype=f32).reshape(3, 4)
    return bool(np.array_equal(m, rigid()))


def apply_rigid(positions, normals, m):
    """Positions (and vertex normals, or None) of a mesh moved by the 3x4 `m` as the device moves them:

        p'_r = fl(fl(fl(fl(m_r0 x) + fl(m_r1 y)) + fl(m_r2 z)) + m_r3)       every product and sum rounded to float32
        n'_r = fl(fl(fl(m_r0 nx) + fl(m_r1 ny)) + fl(m_r2 nz))              no translation, not renormalised

    An identity `m` returns the arrays unchanged (bit for bit, signed zeros included).  Returns (positions', normals')."""
    m = np.asarray(m, dtype=f32).reshape(3, 4)
    p = np.ascontiguousarray(positions, dtype=f32).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)
    if is_identity(m):
        return p.copy(), None if n is None else n.copy()

    def rot(v):
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        out = np.empty_like(v)
        for r in range(3):
            a = m[r, 0] * x          # float32 scalar * float32 array: rounded to float32
            b = m[r, 1] * y
            c = m[r, 2] * z
            s = a + b
            out[:, r] = s + c
        return out

    p2 = rot(p)
    p2 += m[:, 3][None, :]
    return p2, None if n is None else rot(n)


def apply_skin(positions, normals, index, weight, bones):
    """Rest positions (and rest normals, or None) of a mesh posed by linear-blend skinning as the device poses them
    (bf_scene_pose_skin): index uint[nv, 4] and weight float32[nv, 4] name four bones per vertex, bones is float32[n_bones, 3, 4].

        q_k = apply_rigid's formula for bones[index[:, k]] on the vertex        k = 0..3, every product and sum rounded
        p'  = fl(fl(fl(fl(w0 q_0) + fl(w1 q_1)) + fl(w2 q_2)) + fl(w3 q_3))     per coordinate
        n'  = the same without the translations, not renormalised

    All four terms are always evaluated (a zero weight still multiplies its bone's result) and an identity bone takes no
    shortcut, so a -0.0 may come out as +0.0.  Returns (positions', normals')."""
    p = np.ascontiguousarray(positions, dtype=f32).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)
    ix = np.asarray(index).reshape(-1, 4).astype(np.int64)
    w = np.ascontiguousarray(weight, dtype=f32).reshape(-1, 4)
    b = np.ascontiguousarray(bones, dtype=f32).reshape(-1, 3, 4)
    if ix.shape[0] != p.shape[0] or w.shape[0] != p.shape[0]:
        raise ValueError(f"{p.shape[0]} vertices, {ix.shape[0]} index rows, {w.shape[0]} weight rows")
    if ix.size and (ix.min() < 0 or ix.max() >= b.shape[0]):
        raise ValueError(f"bone index out of range for {b.shape[0]} bones")

    def blend(v, with_t):
        out = np.empty_like(v)
        x, y, z = v[:, 0], v[:, 1], v[:, 2]
        for k in range(4):                           # the slots in order: per coordinate, ((w0 q0 + w1 q1) + w2 q2) + w3 q3
            m = b[ix[:, k]]                          # [nv, 3, 4] float32: every operation below is float32 on float32
            for r in range(3):
                q = m[:, r, 0] * x
                q = q + m[:, r, 1] * y
                q = q + m[:, r, 2] * z
                if with_t:
                    q = q + m[:, r, 3]
                t = w[:, k] * q
                out[:, r] = t if k == 0 else out[:, r] + t
        return out

    with np.errstate(over="ignore", invalid="ignore"):
        return blend(p, True), None if n is None else blend(n, False)


def bone_dual_quaternions(bones):
    """float32[n_bones, 8]: the unit dual quaternions of rigid bones float32[n_bones, 3, 4], as the library converts the bone table of a
    shape in BF_SKIN_DUAL_QUATERNION (bf_bone_dual_quaternions / capi.bone_dual_quaternions, bit for bit).  float64, rounded to float
    once at the end:

        tr = (m00 + m11) + m22;  the branch is the largest of (tr, m00, m11, m22), the first among equals in that order
        branch tr:   s = sqrt(((1 + m00) + m11) + m22), w = s / 2, f = 0.5 / s, x = (m21 - m12) f, y = (m02 - m20) f, z = (m10 - m01) f
        branch m00:  s = sqrt(((1 + m00) - m11) - m22), x = s / 2, f = 0.5 / s, w = (m21 - m12) f, y = (m01 + m10) f, z = (m02 + m20) f
        branch m11:  s = sqrt(((1 - m00) + m11) - m22), y = s / 2, f = 0.5 / s, w = (m02 - m20) f, x = (m01 + m10) f, z = (m12 + m21) f
        branch m22:  s = sqrt(((1 - m00) - m11) + m22), z = s / 2, f = 0.5 / s, w = (m10 - m01) f, x = (m02 + m20) f, y = (m12 + m21) f
        q = (w, x, y, z) / sqrt(((w w + x x) + y y) + z z), each component divided
        dual = (0, t) q / 2:  dw = -0.5 ((tx x + ty y) + tz z),  dx = 0.5 ((tx w + ty z) - tz y),  dy = 0.5 ((ty w + tz x) - tx z),
                              dz = 0.5 ((tz w + tx y) - ty x)
        out = (w, x, y, z, dw, dx, dy, dz)

    A bone that is not rigid (in float64, max |R^T R - I| <= 1e-4 and det R > 0) or not finite is a ValueError naming it."""
    b = np.ascontiguousarray(bones, dtype=f32).reshape(-1, 3, 4)
    out = np.empty((b.shape[0], 8), f32)
    for k, m in enumerate(b.astype(np.float64)):
        r, t = m[:, :3], m[:, 3]
        if not np.all(np.isfinite(m)):
            raise ValueError(f"bone {k} has a non-finite entry")
        if not (np.abs(r.T @ r - np.eye(3)).max() <= 1e-4 and np.linalg.det(r) > 0.0):
            raise ValueError(f"bone {k} is not rigid")
        (m00, m01, m02), (m10, m11, m12), (m20, m21, m22) = r
        tx, ty, tz = t
        one, half = np.float64(1.0), np.float64(0.5)
        branch = int(np.argmax([(m00 + m11) + m22, m00, m11, m22]))      # argmax: the first among equals
        if branch == 0:
            s = np.sqrt(((one + m00) + m11) + m22)
            f = half / s
            w, x, y, z = s / 2.0, (m21 - m12) * f, (m02 - m20) * f, (m10 - m01) * f
        elif branch == 1:
            s = np.sqrt(((one + m00) - m11) - m22)
            f = half / s
            x, w, y, z = s / 2.0, (m21 - m12) * f, (m01 + m10) * f, (m02 + m20) * f
        elif branch == 2:
            s = np.sqrt(((one - m00) + m11) - m22)
            f = half / s
            y, w, x, z = s / 2.0, (m02 - m20) * f, (m01 + m10) * f, (m12 + m21) * f
        else:
            s = np.sqrt(((one - m00) - m11) + m22)
            f = half / s
            z, w, x, y = s / 2.0, (m10 - m01) * f, (m02 + m20) * f, (m12 + m21) * f
        n = np.sqrt(((w * w + x * x) + y * y) + z * z)
        w, x, y, z = w / n, x / n, y / n, z / n
        out[k] = [w, x, y, z, -half * ((tx * x + ty * y) + tz * z), half * ((tx * w + ty * z) - tz * y),
                  half * ((ty * w + tz * x) - tx * z), half * ((tz * w + tx * y) - ty * x)]
    return out


def apply_skin_dq(positions, normals, index, weight, bones):
    """Rest positions (and rest normals, or None) of a mesh posed by dual-quaternion skinning as the device poses a shape in
    BF_SKIN_DUAL_QUATERNION (Scene.set_skin_mode): apply_skin's arguments, every bone that some vertex weighs rigid.  The table is
    bone_dual_quaternions of those bones and the identity (1, 0, 0, 0; 0, 0, 0, 0) for a bone no vertex weighs.  fp32, every
    operation rounded (no FMA, IEEE division and square root).  Per vertex, with slots k = 0..3:

        p   = the slot of largest weight, the first among equals;   s_k = -1 if dot(D_k.real, D_p.real) < 0, else +1
        b   = ((s0 w0 D_0 + s1 w1 D_1) + s2 w2 D_2) + s3 w3 D_3     per component over all eight, all four terms always evaluated
        r   = b.real / |b.real|,  e = b.dual / |b.real|             (dot and |.|^2 are ((a0 b0 + a1 b1) + a2 b2) + a3 b3)
        rotate(r, v) = (v + rw t) + cross(r.xyz, t)  with  t = 2 cross(r.xyz, v),   cross(a, b).x = fl(fl(ay bz) - fl(az by))
        x'  = rotate(r, x) + 2 ((rw e.xyz - ew r.xyz) + cross(r.xyz, e.xyz))
        n'  = rotate(r, n)                                          no translation, not renormalised

    s_k w_k is exact (a sign), and so are the products by 2.  Returns (positions', normals')."""
    p = np.ascontiguousarray(positions, dtype=f32).reshape(-1, 3)
    n = None if normals is None else np.ascontiguousarray(normals, dtype=f32).reshape(-1, 3)
    ix = np.asarray(index).reshape(-1, 4).astype(np.int64)
    w = np.ascontiguousarray(weight, dtype=f32).reshape(-1, 4)
    b = np.ascontiguousarray(bones, dtype=f32).reshape(-1, 3, 4)
    if ix.shape[0] != p.shape[0] or w.shape[0] != p.shape[0]:
        raise ValueError(f"{p.shape[0]} vertices, {ix.shape[0]} index rows, {w.shape[0]} weight rows")
    if ix.size and (ix.min() < 0 or ix.max() >= b.shape[0]):
        raise ValueError(f"bone index out of range for {b.shape[0]} bones")
    if not np.all(np.isfinite(b)):
        raise ValueError("bones: non-finite entry")
    used = np.zeros(b.shape[0], bool)
    used[ix[w > 0]] = True
    table = np.zeros((b.shape[0], 8), f32)
    table[:, 0] = 1.0
    if used.any():
        try:
            table[used] = bone_dual_quaternions(b[used])
        except ValueError as e:
            raise ValueError(f"{e} (numbered among the bones some vertex weighs: {np.nonzero(used)[0].tolist()})") from None
    rows = np.arange(p.shape[0])
    d = table[ix]                                            # [nv, 4 slots, 8] float32: every operation below is float32 on float32

    def dot4(a, c):
        return ((a[:, 0] * c[:, 0] + a[:, 1] * c[:, 1]) + a[:, 2] * c[:, 2]) + a[:, 3] * c[:, 3]

    def cross(a, c):
        return np.stack([a[:, 1] * c[:, 2] - a[:, 2] * c[:, 1], a[:, 2] * c[:, 0] - a[:, 0] * c[:, 2], a[:, 0] * c[:, 1] - a[:, 1] * c[:, 0]], -1)

    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        pivot = d[rows, np.argmax(w, axis=1), :4]            # argmax: the first among equals
        c = np.stack([np.where(dot4(d[:, k, :4], pivot) < 0, -w[:, k], w[:, k]) for k in range(4)], -1)
        blend = np.stack([((c[:, 0] * d[:, 0, j] + c[:, 1] * d[:, 1, j]) + c[:, 2] * d[:, 2, j]) + c[:, 3] * d[:, 3, j] for j in range(8)], -1)
        length = np.sqrt(dot4(blend[:, :4], blend[:, :4]))
        r, e = blend[:, :4] / length[:, None], blend[:, 4:] / length[:, None]
        two, rw, ew, ru, eu = f32(2.0), r[:, :1], e[:, :1], r[:, 1:], e[:, 1:]

        def rotate(v):
            t = two * cross(ru, v)
            return (v + rw * t) + cross(ru, t)

        p2 = rotate(p) + two * ((rw * eu - ew * ru) + cross(ru, eu))
        return p2.astype(f32, copy=False), None if n is None else rotate(n)


def vertex_normals_f32(positions, faces):
    """The vertex normals the device computes under BF_NORMALS_RECOMPUTE (Scene.set_normal_mode), bit for bit, on the host:
    angle-weighted face normals summed per vertex in increasing face index, every operation fp32 (the statement is in
    include/beifong_hip.h; this is bf_vertex_normals, which needs no device).  Put them into a description so that frame 0
    matches the frames the device recomputes.  A vertex of no face, or of degenerate faces only, gets (1, 0, 0).
    positions float32[nv, 3], faces uint32[nf, 3] -> float32[nv, 3]."""
    from . import capi
    return capi.vertex_normals(positions, faces)


def apply_morph(rest, rest_normals, delta_positions, delta_normals, weights):
    """Rest positions (and rest normals, or None) of a mesh moved by morph targets as the device moves them (bf_scene_pose_morph):
    delta_positions float32[n_targets, nv, 3], delta_normals the same shape or None, weights float32[n_targets].

        p = rest;  for k in increasing order:  p = fl(p + fl(w_k d_k))        per coordinate, every product and sum rounded
        n likewise from the rest normal and the normal deltas, not renormalised

    Every target is always evaluated (a zero weight takes no shortcut, so a -0.0 may come out as +0.0).  With no normal deltas
    the rest normals are returned as they are, bit for bit.  Returns (positions', normals'); the composition with a skin is
    apply_skin(*apply_morph(...), index, weight, bones)."""
    p = np.ascontiguousarray(rest, dtype=f32).reshape(-1, 3).copy()
    n = None if rest_normals is None else np.ascontiguousarray(rest_normals, dtype=f32).reshape(-1, 3).copy()
    w = np.ascontiguousarray(weights, dtype=f32).reshape(-1)
    dp = np.ascontiguousarray(delta_positions, dtype=f32).reshape(w.shape[0], -1, 3)
    if dp.shape[1] != p.shape[0]:
        raise ValueError(f"{p.shape[0]} vertices, deltas for {dp.shape[1]}")
    dn = None
    if delta_normals is not None:
        if n is None:
            raise ValueError("normal deltas without rest normals")
        dn = np.ascontiguousarray(delta_normals, dtype=f32).reshape(w.shape[0], -1, 3)
        if dn.shape != dp.shape:
            raise ValueError(f"delta_normals {dn.shape}, delta_positions {dp.shape}")
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(w.shape[0]):                  # float32 on float32: each product and each sum is rounded once
            p = p + w[k] * dp[k]
            if dn is not None:
                n = n + w[k] * dn[k]
    return p, n


def moved_description(sd, transforms):
    """A new SceneDesc equal to `sd` with every mesh's positions and normals replaced by apply_rigid(..., transforms[k]):
    the scene bf_scene_create would have to rebuild for the pose bf_scene_transform_meshes gives a handle of `sd`.
    `transforms`: float[n_shapes, 3, 4].  Indices, texture coordinates, materials and endpoints are `sd`'s (kept alive)."""
    import ctypes as C

    from . import capi
    from .scenedesc import SceneDesc
    xf = np.asarray(transforms, dtype=f32).reshape(len(sd.shapes), 3, 4)
    out = SceneDesc()
    C.memmove(C.byref(out.physics), C.byref(sd.physics), C.sizeof(capi.bf_physics))
    C.memmove(C.byref(out.sensor), C.byref(sd.sensor), C.sizeof(capi.bf_sensor))
    out.materials, out.emitters = list(sd.materials), list(sd.emitters)
    out._keep.append(sd)
    for k, s in enumerate(sd.shapes):
        s2 = capi.bf_shape()
        C.memmove(C.byref(s2), C.byref(s), C.sizeof(capi.bf_shape))
        if s.type == capi.BF_SHAPE_MESH and s.n_vertices and not is_identity(xf[k]):
            p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3))
            n = np.ctypeslib.as_array(s.normals, shape=(s.n_vertices, 3)) if s.normals else None
            p2, n2 = apply_rigid(p, n, xf[k])
            out._keep += [p2, n2]
            s2.positions = p2.ctypes.data_as(C.POINTER(C.c_float))
            if n2 is not None:
                s2.normals = n2.ctypes.data_as(C.POINTER(C.c_float))
        out.shapes.append(s2)
    return out.finalize()


def deformed_description(sd, vertices):
    """A new SceneDesc equal to `sd` with the arrays named in `vertices` replaced: {shape: positions} or
    {shape: (positions, normals)}, float32 [n_vertices, 3] each (normals None: the mesh keeps the ones it has).  The scene
    bf_scene_create would have to rebuild for the base bf_scene_update_vertices gives a handle of `sd`; composes with
    moved_description (deform first, then move: the pose is applied on top of the new base).  Indices, texture coordinates,
    materials and endpoints are `sd`'s (kept alive); nothing is converted: the arrays must be float32 already."""
    import ctypes as C

    from . import capi
    from .scenedesc import SceneDesc
    out = SceneDesc()
    C.memmove(C.byref(out.physics), C.byref(sd.physics), C.sizeof(capi.bf_physics))
    C.memmove(C.byref(out.sensor), C.byref(sd.sensor), C.sizeof(capi.bf_sensor))
    out.materials, out.emitters = list(sd.materials), list(sd.emitters)
    out._keep.append(sd)
    todo = {int(k): v for k, v in vertices.items()}
    for k in todo:
        if not 0 <= k < len(sd.shapes):
            raise ValueError(f"shape index {k} out of range for a scene of {len(sd.shapes)} shapes")
    for k, s in enumerate(sd.shapes):
        s2 = capi.bf_shape()
        C.memmove(C.byref(s2), C.byref(s), C.sizeof(capi.bf_shape))
        if k in todo:
            if s.type != capi.BF_SHAPE_MESH:
                raise ValueError(f"shape {k} is not a mesh")
            v = todo[k]
            p, n = v if isinstance(v, tuple) else (v, None)
            p = capi.vertex_array(p, f"positions of shape {k}", s.n_vertices)
            out._keep.append(p)
            s2.positions = p.ctypes.data_as(C.POINTER(C.c_float))
            if n is not None:
                if not s.normals:
                    raise ValueError(f"shape {k} has no vertex normals: it cannot take any")
                n = capi.vertex_array(n, f"normals of shape {k}", s.n_vertices)
                out._keep.append(n)
                s2.normals = n.ctypes.data_as(C.POINTER(C.c_float))
        out.shapes.append(s2)
    return out.finalize()
