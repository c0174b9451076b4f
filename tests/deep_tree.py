"""Inputs that drive a lane's traversal stack past its LDS part, and a CPU walker that measures how far (no GPU, no expected values).

A lane's stack keeps its first 16 (wf_trace) or 32 (bf_render_kernel, the tail's traverse_quad, bf_trace_kernel) entries in LDS and
the rest in a per-thread HBM column (bf_device_core.h: LaneStack).  bf_scene_info.bvh_stack_need is the worst case over all rays;
random rays on any mesh of the suite keep 0 to 2 entries alive, so only inputs made for it reach the overflow path:

cone_of_plates(n, r)   triangle k is the right-angled plate (x, 0, 0), (x, x, 0), (x, 0, x) in the plane x = r^-k: every plate's box
                       contains the boxes of all smaller ones, and the corner of each box opposite the right angle is empty.  Triangle
                       0's first vertex is moved to (1, 1, 1): it covers that far corner instead, the backstop.
apex_rays(k)           from just behind the apex along (1, a, a), a in [0.6, 0.95]: through the empty corner of every plate's box, so
                       nearest-first traversal descends the whole chain, keeping the far children of every level, and hits nothing
                       but the backstop (t ~ 1.32 .. 1.68) at the very end.
climbing_rays(n, r)    from inside the corner, just above the apex, along (1, s, s) with small s: as deep, but answered by a plate next to
                       the apex, whose leaf hangs off one of the LAST entries pushed.  An apex ray's answer never depends on what the
                       overflow part of its stack holds; these rays' answers do (needs_entries_from counts them).
stack_occupancy        the kernels' walk (node4_decide / leaf_intersect / the pop rule of traverse_dyn) over the arrays
                       capi.Scene.read_bvh(4) returns, in float32; returns the largest number of live stack entries per ray.  The
                       fused multiply-adds are evaluated in float64 and rounded once more to float32 (a product of two float32 is
                       exact in float64), which differs from a true fma only within 2^-29 of a rounding tie: the walker measures
                       how deep the inputs go, it never supplies a value a kernel is compared with.
"""
import numpy as np

f32 = np.float32
f64 = np.float64

EMPTY = -(1 << 31)          # kNoNode: Node4's empty-child marker, and "traversal finished"
MISS_KEY = 0x7f000000       # kMissKey
EPS = f32(1500 * 2.0 ** -24)
APEX_MINT = f32(1e-4)


def cone_of_plates(n, r):
    """(v float32[3n, 3], f int32[n, 3]): n plates, plate k in the plane x = r^-k, plate 0 the backstop."""
    x = (f64(r) ** -np.arange(n, dtype=f64)).astype(f32)
    v = np.zeros((n, 3, 3), f32)
    v[:, :, 0] = x[:, None]
    v[:, 1, 1] = x
    v[:, 2, 2] = x
    v[0, 0] = [1.0, 1.0, 1.0]
    return np.ascontiguousarray(v.reshape(-1, 3)), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def apex_directions(k):
    a = np.linspace(0.6, 0.95, k)
    d = np.stack([np.ones(k), a, a], 1)
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _rows8(o, mint, d, maxt):
    n = len(o)
    return np.concatenate([o, np.full((n, 1), mint), d, np.full((n, 1), maxt)], 1).astype(f32)


def apex_rays(k, maxt=np.inf):
    """float32[k, 8] = o, mint, d, maxt: from -0.01 d along d = (1, a, a) / |(1, a, a)|"""
    d = apex_directions(k)
    return _rows8(-0.01 * d, APEX_MINT, d, maxt)


def reversed_rays(k):
    """the apex rays walked the other way: from 4 d towards the apex; they meet the backstop first"""
    d = apex_directions(k)
    return _rows8(4.0 * d, APEX_MINT, -d, np.inf)


def climb_origin(n, r):
    """a point in the empty corner of every plate's box, half-way between the apex and the smallest plate"""
    x0 = 0.5 * f64(r) ** -(n - 1)
    return np.array([x0, 0.9 * x0, 0.9 * x0])


def climbing_rays(n, r, k=256):
    """float32[k, 8]: from climb_origin along (1, s, s), s in [0, 0.35].  y + z grows more slowly than x along such a ray, so it leaves
    the empty corners after a few of the smallest plates and its closest hit is one of the plates next to the apex: the leaves that
    hang off the LAST entries a deep descent pushed.  These are the rays whose answer is read out of the overflow part of the stack
    (needs_entries_from); an apex ray's answer never is."""
    s = np.linspace(0.0, 0.35, k)
    d = np.stack([np.ones(k), s, s], 1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _rows8(np.tile(climb_origin(n, r), (k, 1)), f32(1e-7), d, np.inf)


def random_rays(n, seed, extent=1.5):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-extent, extent, (n, 3))
    d = rng.standard_normal((n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return _rows8(o, EPS, d, np.inf)


def _fma(a, b, c):
    return (np.asarray(a, f64) * np.asarray(b, f64) + np.asarray(c, f64)).astype(f32)


def _cross(a, b):
    # bf_device_math.h: cross = fmsub(a.y, b.z, a.z * b.y), ...
    return np.stack([_fma(a[:, 1], b[:, 2], -(a[:, 2] * b[:, 1])), _fma(a[:, 2], b[:, 0], -(a[:, 0] * b[:, 2])),
                     _fma(a[:, 0], b[:, 1], -(a[:, 1] * b[:, 0]))], 1)


def _dot(a, b):
    return _fma(a[:, 2], b[:, 2], _fma(a[:, 1], b[:, 1], a[:, 0] * b[:, 0]))


def _tri_intersect(p, o, d, mint, maxt):
    """bf_device_core.h: tri_intersect; p float32[m, 3, 3] -> (hit, t)"""
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    pvec = _cross(d, e2)
    inv_det = f32(1.0) / _dot(e1, pvec)
    tvec = o - p[:, 0]
    u = _dot(tvec, pvec) * inv_det
    qvec = _cross(tvec, e1)
    v = _dot(d, qvec) * inv_det
    t = _dot(e2, qvec) * inv_det
    return (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= mint) & (t <= maxt), t


LOST = EMPTY + 1            # _walk(lose_from=k): what a stack position >= k holds


def _walk(nodes, rows, root, rays, any_hit, lose_from=None):
    """The kernels' traversal of every ray: (peak, peak_at_visit, best_t, found).  lose_from=k: an entry pushed at position k or
    above is lost (popping it continues with the entry below), the walk of a stack whose overflow part forgets."""
    rays = np.ascontiguousarray(rays, f32).reshape(-1, 8)
    n = len(rays)
    peak, peak_visit = np.zeros(n, np.int64), np.zeros(n, np.int64)
    best, found = np.full(n, np.inf, f32), np.zeros(n, bool)
    if n == 0 or root == EMPTY or len(rows) == 0:
        return peak, peak_visit, best, found
    o, mint, d, maxt = rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7]
    tri = np.ascontiguousarray(rows[:, :, :3], f32)
    with np.errstate(all="ignore"):
        # ray_inverse: zero components to +-1e30, origin folded in
        inv = np.clip(f32(1.0) / d, f32(-1.0e30), f32(1.0e30)).astype(f32)
        oid = (-o * inv).astype(f32)
        lo = np.stack([nodes["lox"], nodes["loy"], nodes["loz"]], 1) if len(nodes) else np.zeros((0, 3, 4), f32)      # [n_nodes, axis, slot]
        hi = np.stack([nodes["hix"], nodes["hiy"], nodes["hiz"]], 1) if len(nodes) else np.zeros((0, 3, 4), f32)
        child = nodes["child"].astype(np.int64) if len(nodes) else np.zeros((0, 4), np.int64)
        node = np.full(n, int(root), np.int64)
        sp = np.zeros(n, np.int64)
        stack = np.zeros((n, 3 * 31 + 4), np.int64)

        def pop(idx):
            while len(idx):
                has = sp[idx] > 0
                sp[idx[has]] -= 1
                node[idx] = np.where(has, stack[idx, np.maximum(sp[idx], 0)], EMPTY)
                idx = idx[node[idx] == LOST]

        while True:
            live = node != EMPTY
            if not live.any():
                break
            ii = np.flatnonzero(live & (node >= 0))
            il = np.flatnonzero(live & (node < 0))
            if len(ii):
                nd = node[ii]
                tmax = maxt[ii] if any_hit else np.fmin(maxt[ii], best[ii])
                t0 = _fma(lo[nd], inv[ii][:, :, None], oid[ii][:, :, None])      # [m, axis, slot]
                t1 = _fma(hi[nd], inv[ii][:, :, None], oid[ii][:, :, None])
                mn, mx = np.fmin(t0, t1), np.fmax(t0, t1)
                tn = np.fmax(np.fmax(mn[:, 0], mn[:, 1]), np.fmax(mn[:, 2], mint[ii][:, None]))
                tf = np.fmin(np.fmin(mx[:, 0], mx[:, 1]), np.fmin(mx[:, 2], tmax[:, None]))
                hit = tn <= tf * f32(1.0000004)
                ch = child[nd]
                hit[:, 2:] &= ch[:, 2:] != EMPTY
                bits = np.minimum(tn.astype(f32).view(np.uint32).astype(np.int64), MISS_KEY - 4)
                key = np.where(hit, bits & ~3, MISS_KEY) | np.arange(4)[None, :]      # child_key
                order = np.argsort(key, axis=1)
                key = np.take_along_axis(key, order, 1)
                ch = np.take_along_axis(ch, order, 1)
                pushing = key[:, 1] < MISS_KEY
                peak_visit[ii[pushing]] = np.maximum(peak_visit[ii[pushing]], sp[ii[pushing]])
                for j in (3, 2, 1):                                                   # the far ones, farthest first
                    m = key[:, j] < MISS_KEY
                    at = sp[ii[m]]
                    stack[ii[m], at] = ch[m, j] if lose_from is None else np.where(at >= lose_from, LOST, ch[m, j])
                    sp[ii[m]] += 1
                peak[ii] = np.maximum(peak[ii], sp[ii])
                near = key[:, 0] < MISS_KEY
                node[ii[near]] = ch[near, 0]
                pop(ii[~near])
            if len(il):
                enc = (~node[il]) & 0xffffffff
                first, cnt = enc >> 3, (enc & 7) + 1
                done = np.zeros(len(il), bool)
                for j in range(int(cnt.max())):
                    m = cnt > j
                    h, t = _tri_intersect(tri[first[m] + j], o[il[m]], d[il[m]], mint[il[m]], maxt[il[m]])
                    k = il[m][h]
                    best[k] = np.minimum(best[k], t[h])
                    done[np.flatnonzero(m)[h]] = True
                found[il[done]] = True
                if any_hit:
                    node[il[done]] = EMPTY
                    pop(il[~done])
                else:
                    pop(il)
    return peak, peak_visit, best, found


def stack_occupancy(nodes, rows, root, rays, any_hit=False, at_visit=False):
    """The largest number of live stack entries of every ray of `rays` (float32[n, 8]) on the four-wide tree (nodes, rows, root) as
    capi.Scene.read_bvh(4) returns it: int64[n].  any_hit=False narrows the segment to min(maxt, best) as a closest-hit query does;
    any_hit=True keeps maxt and ends at the first hit.  at_visit=True returns instead the largest count a ray had when it came to a
    node at which it then pushed something (LaneStack::push3 leaves its three unconditional LDS writes once that count exceeds
    N_LDS - 3)."""
    return _walk(nodes, rows, root, rays, any_hit)[1 if at_visit else 0]


def needs_entries_from(nodes, rows, root, rays, k, any_hit=False):
    """bool[n]: the rays whose answer (the closest hit's distance, or whether anything is hit) changes when the stack loses every
    entry it holds at position k or above: the rays that find their hit through the overflow part of a stack of k LDS entries.  A ray
    may go deep and not be one of them: an apex ray's only hit, the backstop, waits near the bottom of its stack."""
    _, _, t0, f0 = _walk(nodes, rows, root, rays, any_hit)
    _, _, t1, f1 = _walk(nodes, rows, root, rays, any_hit, lose_from=k)
    return (f0 != f1) | (t0.view(np.uint32) != t1.view(np.uint32))


# ---- scenes around a mesh at the cone's place (descriptions only: no GPU) -------------------------------------------------------------
AXIS = apex_directions(3)[1]          # (1, 0.775, 0.775) / |.|: the middle apex direction
FOV = 8.0                             # degrees: every primary ray is (1, b, c) with b, c within 0.775 +- 0.15, an apex direction
# The sensor's rays share one origin, so it has to sit at the apex on the scale of the smallest plate (1.01^-959 = 7.2e-5): from 0.01
# behind it, as the apex rays of the queries start, oblique rays enter the small boxes outside their empty corner and end there.
EYE = -1e-6 * AXIS


def _xyz(p):
    return [float(x) for x in p]


def flat_plates(n):
    """n small triangles (3 n vertices, as the cone has) on a square grid in the plane x = 1 over y, z in [0, 1]: a balanced, shallow
    tree, in the view of the cone scenes' sensor."""
    side = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    o = np.stack([np.ones(n), (k % side) / side, (k // side) / side], 1).astype(f32)
    s = f32(0.8 / side)
    v = np.stack([o, o + np.array([0, s, 0], f32), o + np.array([0, 0, s], f32)], 1).astype(f32)
    return np.ascontiguousarray(v.reshape(-1, 3)), np.arange(3 * n, dtype=np.int32).reshape(-1, 3)


def render_scene(v, f, n_paths=4096, seed=5, climb=None):
    """(sd, lp, mesh shape): the mesh, a point emitter and a perspective sensor; range mode.
    climb=None: the sensor just behind the apex looks down the axis.  The backstop answers every primary ray after the deep descent; its
    shadow rays run back down the cone to the emitter.
    climb=(n, r): the sensor at climb_origin(n, r) looks along (1, 0.2, 0.2) with a field of view of 10 degrees: its primary rays are
    (1, s, t) with s, t within 0.2 +- 0.09, climbing rays, answered by the plates next to the apex."""
    from beifong_amd import capi
    from beifong_amd.scenedesc import SceneDesc, Transform4f as T
    sd = SceneDesc()
    mesh = sd.add_mesh(v, f, sd.add_diffuse(0.8, twosided=True))
    if climb is None:
        sd.add_point(_xyz(2.0 * EYE), intensity=10.0)
        sd.set_perspective(T.look_at(_xyz(EYE), _xyz(AXIS), [0, 0, 1]), fov=FOV, near_clip=1e-5, far_clip=100.0)
    else:
        eye = climb_origin(*climb)
        sd.add_point(_xyz(eye * [0.9, 1.0, 1.0]), intensity=1e-6)
        sd.set_perspective(T.look_at(_xyz(eye), _xyz(eye + [1.0, 0.2, 0.2]), [0, 0, 1]), fov=10.0, near_clip=1e-6, far_clip=100.0)
    sd.finalize()
    return sd, capi.make_launch(capi.BF_MODE_RANGE, n_paths, seed=seed, bins=64, bin_width=0.1, color_mode=capi.BF_COLOR_RGB), mesh


RX_HALF = 2e-7                        # half the side of the receive scene's apertures


def receive_scene(v, f, n_paths=4096, seed=6, t_bins=64):
    """(sd, lp): the mesh with a Wigner transmitter and a Wigner receiver on two coincident rectangles just behind the apex, facing down
    the axis (endpoints as tests/scene_builders.py: _zoo_scene's); raw receive mode.  The receiver's rays leave over a cosine hemisphere
    about the axis, so only those inside the cone's corner are apex rays (receiver_rays)."""
    from beifong_amd import capi
    from beifong_amd.scenedesc import SceneDesc, Transform4f as T
    sd = SceneDesc()
    c, lmin, lmax = sd.physics.c, sd.physics.lambda_min_nm, sd.physics.lambda_max_nm
    pose = T.look_at(_xyz(EYE), _xyz(EYE + AXIS), [0, 0, 1]) * T.scale([RX_HALF, RX_HALF, 1])
    txa = sd.add_rectangle(pose, sd.add_diffuse(0.0))
    rxa = sd.add_rectangle(pose, sd.add_diffuse(0.5))
    tau = 2.0 * 0.1 / c
    f_c = c / (0.5 * (lmin + lmax) * 1e-9)
    sd.add_wigner_transmitter(txa, signaltype="pulse", amplitude=1.0, freq_centre=f_c, freq_ext=1.0 / tau, pulse_len=tau,
                              prf=1.0 / (t_bins * tau), gain=1.0)
    sd.set_receiver(rxa, kind="wigner", adc_sampling_start=0.0, adc_sampling_end=t_bins * tau, t_bins=t_bins, f_bins=1,
                    t_bandwidth=t_bins * tau, f_bandwidth=2.0 * c / (lmin * 1e-9), freq_centre=f_c,
                    freq_ext=c / (lmin * 1e-9) - c / (lmax * 1e-9))
    sd.add_mesh(v, f, sd.add_diffuse(0.8, twosided=True))
    sd.finalize()
    return sd, capi.make_launch(capi.BF_MODE_RECEIVE_RAW, n_paths, seed=seed, bins=t_bins, bins_y=1)


def receiver_rays(n, seed):
    """float32[n, 8]: rays as the receive scene's receiver starts them (a point of the aperture, a cosine-weighted direction about the
    axis, mint as the kernels' kRayEpsilon), drawn here with numpy: the same distribution, not the render's own sample sequence."""
    rng = np.random.default_rng(seed)
    s = AXIS[[1, 0, 2]] * [-1, 1, 0]
    s /= np.linalg.norm(s)
    t = np.cross(AXIS, s)
    u = rng.random((n, 4))
    r, phi = np.sqrt(u[:, 0]), 2.0 * np.pi * u[:, 1]
    d = (r * np.cos(phi))[:, None] * s + (r * np.sin(phi))[:, None] * t + np.sqrt(1.0 - u[:, 0])[:, None] * AXIS
    o = EYE + RX_HALF * ((2.0 * u[:, 2] - 1.0)[:, None] * s + (2.0 * u[:, 3] - 1.0)[:, None] * t)
    return _rows8(o, EPS, d, np.inf)


def film_grid(side=16):
    """float32[side^2, 4] rows of Scene.sensor_sample_ray: film positions on a grid that includes the film's corners, aperture (0.5, 0.5)"""
    u = np.linspace(0.0, 1.0, side)
    fx, fy = np.meshgrid(u, u)
    return np.stack([fx.ravel(), fy.ravel(), np.full(side * side, 0.5), np.full(side * side, 0.5)], 1).astype(f32)


def sensor_rays(sample_rows):
    """float32[n, 8] rays from the float32[n, 9] rows Scene.sensor_sample_ray returns (o, mint, d, weight, maxt)"""
    r = np.asarray(sample_rows, f32)
    return np.ascontiguousarray(np.concatenate([r[:, 0:7], r[:, 8:9]], 1))


