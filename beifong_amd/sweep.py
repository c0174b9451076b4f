"""Frame sweeps: the reference's radar scripts render one frame per radar pose or pulse in a Python
loop that rebuilds the whole scene every time (python_scripts/animated_trans_rad.py:307-384,
Receive.ipynb cell 30).  Here the frames of a sweep

  * rotate over `n_streams` HIP streams, one device scene handle each, so that the latency-bound
    deep-path tail of one frame overlaps the heads of the next ones;
  * keep the BVH on the device while only endpoints move: a frame whose mesh arrays are the very
    arrays of the handle's previous frame is applied with bf_scene_update_endpoints (rectangle
    transforms, emitter / transmitter, sensor / receiver records — microseconds instead of a rebuild).

Needs torch only for device buffers and streams.
"""
import ctypes as C

import numpy as np

from . import capi


def geometry_key(sd):
    """Identity of a description's meshes: the addresses and sizes of the arrays it points to."""
    key = []
    for s in sd.shapes:
        if s.type == capi.BF_SHAPE_MESH:
            key.append((C.cast(s.positions, C.c_void_p).value, s.n_vertices, C.cast(s.indices, C.c_void_p).value, s.n_faces,
                        C.cast(s.normals, C.c_void_p).value))
        else:
            key.append(None)
    return tuple(key)


def render_sweep(frames, n_streams=4, lib=None, device=None, rolling=True):
    """Render `frames` — an iterable of (SceneDesc, bf_launch) — and return float32[n_frames, channels].

    All frames must produce the same number of channels.  Frames are independent renders; their
    order in the output is the input order.  rolling (round 4): the frames a handle renders form ONE rolling
    sequence — an endpoint update between two frames joins it (bf_scene_update_endpoints) — flushed once at the end,
    so a sweep whose radar turns per frame (animated_trans_rad.py:307-384) pays one tail per handle, not one per frame."""
    import torch
    lib = lib or capi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    streams = [torch.cuda.Stream(dev) for _ in range(n_streams)]
    handles = [None] * n_streams
    keys = [None] * n_streams
    hists = []
    stats = {"created": 0, "updated": 0}
    for k, (sd, lp) in enumerate(frames):
        j = k % n_streams
        key = geometry_key(sd)
        with torch.cuda.stream(streams[j]):
            if handles[j] is not None and keys[j] == key:
                handles[j].update_endpoints(sd, stream=streams[j].cuda_stream)
                stats["updated"] += 1
            else:
                if handles[j] is not None:
                    # the old handle's rolling sequence is still open: finish its paths (bf_scene_destroy abandons them), and
                    # let its last render be done before it goes
                    handles[j].flush(stream=streams[j].cuda_stream)
                    streams[j].synchronize()
                    handles[j].close()
                handles[j] = capi.Scene(sd, lib)
                keys[j] = key
                stats["created"] += 1
            h = torch.zeros(handles[j].channels(lp), dtype=torch.float32, device=dev)
            multi_pixel = lp.spp and lp.film_width and lp.film_height
            if rolling and not multi_pixel and not (lp.flags & capi.BF_FLAG_MEGAKERNEL):
                lr = capi.bf_launch()
                C.memmove(C.byref(lr), C.byref(lp), C.sizeof(capi.bf_launch))
                lr.flags |= capi.BF_FLAG_ROLLING
                lp = lr
            handles[j].render_device(lp, h.data_ptr(), stream=streams[j].cuda_stream)
            hists.append(h)
    for j, hd in enumerate(handles):
        if hd is not None:
            hd.flush(stream=streams[j].cuda_stream)
    for s in streams:
        s.synchronize()
    out = np.stack([h.cpu().numpy() for h in hists]) if hists else np.zeros((0, 0), np.float32)
    for h in handles:
        if h is not None:
            h.close()
    render_sweep.last_stats = stats
    return out


def _shard_launch(launch, off, cnt):
    lp = capi.bf_launch()
    C.memmove(C.byref(lp), C.byref(launch), C.sizeof(capi.bf_launch))
    lp.path_offset = launch.path_offset + off
    lp.n_paths = cnt
    return lp


class PulseSweeper:
    """Device-resident state of a pulse sweep: ONE scene (one BVH build) and `n_streams` HIP streams, kept across
    sweeps.  The pulses of a sweep are rendered as `n_streams` BATCHES (bf_render_batch_device): each batch is one
    launch sequence over its pulses — the pulse's mesh offset is added to the triangles on the fly and the cube is
    accumulated with atomics — so a sweep pays one latency-bound tail per batch instead of one per pulse, and the
    batches' tails overlap each other's heads.  See render_pulse_sweep."""

    def __init__(self, sd, launch, n_streams=2, lib=None, device=None):
        from . import configure_runtime
        configure_runtime()          # hardware queues per process (no effect once HIP has started)
        import torch
        self.lib = lib or capi.load_library()
        self.dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.launch = launch
        self.n_streams = max(1, int(n_streams))
        self.streams = [torch.cuda.Stream(self.dev) for _ in range(self.n_streams)]
        # one handle per stream: a handle owns the path pool its renders run in (the BVH build is shared work only
        # through bf_scene_clone, see capi.Scene.clone)
        first = capi.Scene(sd, self.lib)
        self.handles = [first] + [first.clone() for _ in range(self.n_streams - 1)]
        self.n_chan = self.handles[0].channels(launch)

    def render(self, offsets, group=None, per_pulse=False):
        """float32[n_pulses, f_bins * t_bins, 3] of (I, Q, W) for target offsets float[n_pulses, 3].
        per_pulse=True renders pulse by pulse (bf_scene_translate_meshes + one render each): the round-1 path, kept
        as the reference the batched path is tested against."""
        import torch
        import torch.distributed as tdist
        from .dist import render_cube_sharded
        offsets = np.ascontiguousarray(np.asarray(offsets, dtype=np.float32).reshape(-1, 3))
        n = len(offsets)

        def render(path_off, count, cube):
            lp = _shard_launch(self.launch, path_off, count)
            # the cube was zero-filled on the current stream: the side streams must not start before that
            for s in self.streams:
                s.wait_stream(torch.cuda.current_stream(self.dev))
            if per_pulse:
                for k, off in enumerate(offsets):
                    j = k % self.n_streams
                    with torch.cuda.stream(self.streams[j]):
                        self.handles[j].translate_meshes(off, stream=self.streams[j].cuda_stream)
                        self.handles[j].render_device(lp, cube[k].data_ptr(), stream=self.streams[j].cuda_stream)
                for j in range(self.n_streams):         # leave the handles as built
                    with torch.cuda.stream(self.streams[j]):
                        self.handles[j].translate_meshes((0.0, 0.0, 0.0), stream=self.streams[j].cuda_stream)
            else:
                bounds = [n * j // self.n_streams for j in range(self.n_streams + 1)]
                for j in range(self.n_streams):
                    k0, k1 = bounds[j], bounds[j + 1]
                    if k1 == k0:
                        continue
                    with torch.cuda.stream(self.streams[j]):
                        self.handles[j].render_batch_device(lp, k1 - k0, cube[k0].data_ptr(), offsets=offsets[k0:k1],
                                                            stream=self.streams[j].cuda_stream)
            for s in self.streams:
                s.synchronize()

        cube, _ = render_cube_sharded(render, int(self.launch.n_paths), (n, self.n_chan), device=self.dev,
                                      group=group if tdist.is_initialized() else None)
        return cube.cpu().numpy().reshape(n, -1, 3)

    def close(self):
        for h in reversed(self.handles):
            h.close()
        self.handles = []


def render_pulse_sweep(sd, launch, offsets, n_streams=2, lib=None, device=None, group=None):
    """Coherent pulse sweep over a rigidly moving target (BASELINE configs[4]).

    `sd`      scene description whose meshes are the target (rectangles — ground, antennas — stay put);
    `launch`  a BF_MODE_RECEIVE_IQ launch; every pulse uses the SAME seed (common random numbers), so a
              path keeps its geometry from pulse to pulse and only its optical length — its phase — moves;
    `offsets` float[n_pulses, 3]: target offset of each pulse, relative to the scene as built.

    The BVH is built once; the pulses are rendered in `n_streams` batches (bf_render_batch_device: the pulse's offset
    is applied to the triangles on the fly, every path bit-identical to a render of the translated scene).  Returns the slow-time x fast-time
    cube float32[n_pulses, f_bins * t_bins, 3] of (I, Q, W).  One-shot form of PulseSweeper (which keeps the
    handles for further sweeps).

    Under an initialised torch.distributed job (one process per GPU) every rank renders its contiguous share of
    each pulse's paths (bf_launch.path_offset) and the cube is summed with one all-reduce at the end
    (beifong_amd.dist.render_cube_sharded); every rank returns the full cube."""
    n = len(np.asarray(offsets, dtype=np.float32).reshape(-1, 3))
    sw = PulseSweeper(sd, launch, max(1, min(n_streams, n)), lib, device)
    try:
        return sw.render(offsets, group)
    finally:
        sw.close()


def _classed(first, launch, classes):
    """classes = (shape_class, n_classes, miss_class), a capi.bf_arrival_bins (classes by direction of arrival), a pair
    (capi.bf_range_rate_bins, twists) (classes by range rate) or None -> (the launch to render, n_classes or 0): the table goes
    onto `first` (its clones inherit it) and the launch carries BF_FLAG_CLASSES."""
    if classes is None:
        return launch, 0
    if isinstance(classes, capi.bf_arrival_bins):
        first.set_arrival_classes(classes)
    elif len(classes) == 2 and isinstance(classes[0], capi.bf_range_rate_bins):
        first.set_range_rate_classes(*classes)
    else:
        shape_class, n_classes, miss_class = classes
        first.set_classes(shape_class, n_classes, miss_class)
    lc = capi.bf_launch.from_buffer_copy(launch)
    lc.flags |= capi.BF_FLAG_CLASSES
    return lc, first.channels(lc) // first.channels(launch)


def _every(rebuild_every):
    if rebuild_every is not None and int(rebuild_every) < 1:
        raise ValueError("rebuild_every must be a positive integer or None")
    return None if rebuild_every is None else int(rebuild_every)


def _transforms(transforms, n):
    """The optional `transforms` of a sweep of n pulses as float32[n, n_shapes, 3, 4], or None."""
    if transforms is None:
        return None
    xf = np.asarray(transforms, dtype=np.float32)
    if xf.ndim != 4 or xf.shape[2:] != (3, 4) or xf.shape[0] != n:
        raise ValueError(f"transforms must be [{n}, n_shapes, 3, 4], got {xf.shape}")
    return xf


def _meshes_of(sd, shapes):
    for k in shapes:
        if not 0 <= int(k) < len(sd.shapes) or sd.shapes[int(k)].type != capi.BF_SHAPE_MESH:
            raise ValueError(f"shape {int(k)} is not a mesh of this scene")


def _rest_pose(sd, shape):
    """(positions [nv, 3], vertex normals [nv, 3] or None) of mesh `shape` as `sd` describes it: views of the description's arrays."""
    s = sd.shapes[int(shape)]
    return (np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)),
            np.ctypeslib.as_array(s.normals, shape=(s.n_vertices, 3)) if s.normals else None)


def _version_sweep(sd, launch, n, xf, n_streams, per_pulse, every, classes, recompute_normals, lib, device, prepare, pose, batch, velocities=None):
    """The driver behind the motion, deform, skin and morph sweeps: `n` pulses of `sd` whose meshes stand at xf[k] (None: as posed)
    on top of what the three callables make of pulse k.

      prepare(first, dev)                          attaches to the first handle, or uploads, what the other two need, before the
                                                   handle is cloned and before the streams wait for the current one;
      pose(handle, k, stream)                      puts the handle's base at pulse k (None: the meshes only move by xf);
      batch(handle, launch, c0, c1, cube_ptr, stream)   the one batched call that renders pulses c0 .. c1 into cube_ptr.

    per_pulse: the pulses rotate over the handles, one pose (+ one bf_scene_transform_meshes) and one render each; else every handle
    renders one contiguous group, in batches of `every` pulses with a rebuild between them if `every` is set.  Returns the cube
    float32[n, f_bins * t_bins, 3], or float32[n, n_classes, f_bins * t_bins, 3] with classes."""
    import torch
    lib = lib or capi.load_library()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
    n_streams = max(1, min(int(n_streams), n))
    if velocities:
        n_streams = 1       # differences are taken between what ONE handle renders: the sweep's own pulse order (_velocities)
    streams = [torch.cuda.Stream(dev) for _ in range(n_streams)]
    first = capi.Scene(sd, lib)
    handles = [first]
    try:
        prepare(first, dev)
        launch, n_classes = _classed(first, launch, classes)
        _recompute(first, recompute_normals)
        _velocities(first, velocities)
        handles += [first.clone() for _ in range(n_streams - 1)]
        cube = torch.zeros((n, handles[0].channels(launch)), dtype=torch.float32, device=dev)
        for s in streams:           # the cube was zero-filled (and prepare's arrays written) on the current stream
            s.wait_stream(torch.cuda.current_stream(dev))
        updates = [0] * n_streams
        if per_pulse:
            for k in range(n):
                j = k % n_streams
                h, stream = handles[j], streams[j].cuda_stream
                with torch.cuda.stream(streams[j]):
                    if pose is not None:
                        pose(h, k, stream)
                    if xf is not None:
                        h.transform_meshes(xf[k], stream=stream)
                    updates[j] += 1
                    if every and updates[j] % every == 0:
                        h.rebuild_bvh(stream=stream)
                    h.render_device(launch, cube[k].data_ptr(), stream=stream)
        else:
            bounds = np.linspace(0, n, n_streams + 1).astype(int)
            for j in range(n_streams):
                lo, hi = int(bounds[j]), int(bounds[j + 1])
                h, stream = handles[j], streams[j].cuda_stream
                for c0 in range(lo, hi, every or max(1, hi - lo)):
                    c1 = min(hi, c0 + every) if every else hi
                    with torch.cuda.stream(streams[j]):
                        if every and c0 > lo:
                            # the k-th frame since the last rebuild has just been rendered: the trees follow the meshes to it
                            pose(h, c0 - 1, stream)
                            h.rebuild_bvh(stream=stream)
                        batch(h, launch, c0, c1, cube[c0].data_ptr(), stream)
        for s in streams:
            s.synchronize()
        if pose is not None:
            for h in handles:
                h.sync()            # a vertex beyond the bound given or derived for it (there is none) would be reported here
        return cube.cpu().numpy().reshape((n, n_classes, -1, 3) if n_classes else (n, -1, 3))
    finally:
        for h in reversed(handles):
            h.close()


def render_motion_sweep(sd, launch, transforms, n_streams=2, lib=None, device=None, per_pulse=False, classes=None, velocities=None):
    """Coherent pulse sweep in which every mesh moves on its own: two targets at different speeds, a
    turning car.

    `sd`          scene description; its meshes as described are the pose the transforms start from;
    `launch`      a BF_MODE_RECEIVE_IQ launch (any mode works); every pulse uses the same seed, as in render_pulse_sweep;
    `transforms`  float[n_pulses, n_shapes, 3, 4]: the rigid transform of every shape at every pulse, absolute from the
                  description (identity for rectangles and for meshes that do not move).

    The scene is built once and the pulses are split into `n_streams` contiguous groups, one per handle (bf_scene_clone)
    and stream.  Each group is ONE motion batch (bf_render_motion_batch_device: a geometry version per pulse, one launch
    sequence and one tail for the group).  per_pulse=True is the reference path: the pulses rotate over the handles, one
    transform (bf_scene_transform_meshes: a BVH refit on the device) and one render per pulse; per-path results are the
    same.  Returns the cube float32[n_pulses, f_bins * t_bins, 3] of (I, Q, W), as render_pulse_sweep does.

    classes=(shape_class, n_classes, miss_class): the returns split by the target each path hit first (BF_FLAG_CLASSES,
    Scene.set_classes); the cube is then float32[n_pulses, n_classes, f_bins * t_bins, 3] and range_doppler(cube[:, k]) the
    range-Doppler map of class k.  classes=capi.arrival_bins(...) or capi.arrival_bins_for(sd, ...): the returns split by the
    direction they arrive from (Scene.set_arrival_classes), same cube shape with n_classes = n_u * n_v + 1: cube[:, k] is the
    range-Doppler map of angle bin k, the cube a range-Doppler-angle cube.  classes=(capi.range_rate_bins(...), twists): the
    returns split by the range rate of the scatterer each path hit first (Scene.set_range_rate_classes), n_classes = n_bins + 2;
    the twists are world-space and the same for every pulse.  Every sweep of this module takes any of the three forms, and with
    the third velocities={shape: dt}: those meshes add the differences of their rendered positions over dt to their twist
    (Scene.set_velocity_mode, BF_VELOCITY_DIFFERENCE).  A sweep with velocities runs on ONE handle and stream, n_streams ignored: the
    differences are forward between the pulses of the batch (the last pulse repeats the field before it; at least two pulses),
    backward between consecutive pulses with per_pulse=True."""
    xf = np.asarray(transforms, dtype=np.float32)
    if xf.ndim != 4 or xf.shape[2:] != (3, 4):
        raise ValueError(f"transforms must be [n_pulses, n_shapes, 3, 4], got {xf.shape}")

    def batch(h, lp, c0, c1, cube_ptr, stream):
        h.render_motion_batch_device(lp, xf[c0:c1], cube_ptr, stream=stream)

    return _version_sweep(sd, launch, xf.shape[0], xf, n_streams, per_pulse, None, classes, None, lib, device,
                          lambda first, dev: None, None, batch, velocities)


def _recompute(first, recompute_normals):
    """recompute_normals=(shapes...) of the deform and skin sweeps: BF_NORMALS_RECOMPUTE on the first handle, before it is cloned
    (clones inherit the modes), so every handle of the sweep, per_pulse=True included, recomputes those shapes' vertex normals on
    the device from each pulse's positions."""
    for k in (recompute_normals or ()):
        first.set_normal_mode(int(k), capi.BF_NORMALS_RECOMPUTE)


def _velocities(first, velocities):
    """velocities={shape: dt} of every sweep that takes classes=(bins, twists): BF_VELOCITY_DIFFERENCE with time step dt on the first
    handle, before it is cloned (clones inherit the modes), so those meshes' range rates carry the differences of their rendered
    positions (Scene.set_velocity_mode; capi.corner_velocities is the statement).  The differences are taken within what ONE handle
    renders, so a sweep with velocities runs on one handle and one stream whatever n_streams says (two handles would each difference
    pulses n_streams apart, or repeat a field at the end of every group): forward between the pulses of its one batch (the last pulse
    repeats the field before it; the sweep needs two pulses), backward between consecutive pulses with per_pulse=True (pulse 0 from
    the description's pose).  With rebuild_every the batched path renders several batches: the last pulse of each repeats a field."""
    for k, dt in (velocities or {}).items():
        first.set_velocity_mode(int(k), capi.BF_VELOCITY_DIFFERENCE, float(dt))


def _dual_quaternion(first, dual_quaternion, skinned):
    """dual_quaternion=(shapes...) of the skin and morph sweeps: BF_SKIN_DUAL_QUATERNION on the first handle, before it is cloned
    (clones inherit the modes), so every handle of the sweep blends those shapes' bones as dual quaternions (Scene.set_skin_mode;
    motion.apply_skin_dq is the statement).  The shapes must be among the `skinned` ones."""
    for k in (dual_quaternion or ()):
        if int(k) not in skinned:
            raise ValueError(f"dual_quaternion names shape {int(k)}, which the sweep does not skin")
        first.set_skin_mode(int(k), capi.BF_SKIN_DUAL_QUATERNION)


def render_deform_sweep(sd, launch, positions, transforms=None, n_streams=2, lib=None, device=None, per_pulse=False, rebuild_every=None,
                        classes=None, recompute_normals=None, velocities=None):
    """Coherent pulse sweep in which meshes DEFORM between the pulses: a walking pedestrian, a vibrating
    panel.  The deforming counterpart of render_motion_sweep.

    `positions`   {shape: float32[n_pulses, n_vertices, 3]}: the vertices of every deforming mesh at every pulse;
    `transforms`  None, or float[n_pulses, n_shapes, 3, 4] as in render_motion_sweep, applied on top.

    The scene is built once; the pulses are split into `n_streams` contiguous groups, one per handle and stream, each ONE
    deform batch (bf_render_deform_batch_device) reading its slices of the vertex arrays, which are uploaded once.
    per_pulse=True is the reference path: the pulses rotate over the handles, one bf_scene_update_vertices_device (+ one
    bf_scene_transform_meshes) and one render per pulse; per-path results are the same.
    rebuild_every=k (an integer): a working handle's trees are rebuilt on the device (bf_scene_rebuild_bvh) after every k-th
    frame's update of that handle, so a mesh that drifts far from its first frame keeps a tree made for where it is; the
    batched path then renders its group in batches of k frames, the handle's base vertices set to the frame before each.
    Results do not change.  recompute_normals=(shapes...): those meshes (which must have vertex normals) get the angle-weighted
    normals of every pulse's positions, computed on the device (Scene.set_normal_mode; motion.vertex_normals_f32 is the
    statement), where by default they keep the normals of the description.
    Returns the cube float32[n_pulses, f_bins * t_bins, 3] of (I, Q, W); with
    classes=(shape_class, n_classes, miss_class), as in render_motion_sweep, float32[n_pulses, n_classes, f_bins * t_bins, 3];
    velocities={shape: dt} with classes=(bins, twists), likewise (one handle and stream then, n_streams ignored)."""
    import torch
    every = _every(rebuild_every)
    n, shapes, pos, _ = capi.deform_tables(positions, None, {k: int(sd.shapes[int(k)].n_vertices) for k in positions if 0 <= int(k) < len(sd.shapes)})
    xf = _transforms(transforms, n)
    bound = max(float(np.abs(p).max()) for p in pos)
    if not np.isfinite(bound):
        raise ValueError("positions: non-finite value")
    bound = max(bound, float(np.finfo(np.float32).tiny))
    dpos = []       # the vertex arrays on the device, uploaded once

    def prepare(first, dev):
        dpos.extend(torch.from_numpy(p).to(dev) for p in pos)

    def pose(h, k, stream):
        for sh, d in zip(shapes, dpos):
            h.update_vertices_device(int(sh), d[k].data_ptr(), None, bound, stream=stream)

    def batch(h, lp, c0, c1, cube_ptr, stream):
        h.render_deform_batch_device(lp, c1 - c0, {int(sh): d[c0].data_ptr() for sh, d in zip(shapes, dpos)}, cube_ptr, bound,
                                     transforms=None if xf is None else xf[c0:c1], stream=stream)

    return _version_sweep(sd, launch, n, xf, n_streams, per_pulse, every, classes, recompute_normals, lib, device, prepare, pose, batch, velocities)


def render_skin_sweep(sd, launch, skins, bones, transforms=None, n_streams=2, per_pulse=False, rebuild_every=None, classes=None, lib=None,
                      device=None, recompute_normals=None, dual_quaternion=None, velocities=None):
    """Coherent pulse sweep in which SKINNED meshes are posed by a few bones per pulse: the counterpart of
    render_deform_sweep whose per-pulse input is [n_bones, 3, 4] floats per mesh, not its vertices.

    `skins`       {shape: (index uint32[n_vertices, 4], weight float32[n_vertices, 4])}: the skin of every posed mesh; its
                  rest pose is the mesh as `sd` describes it (positions, and vertex normals if it has any);
    `bones`       {shape: float32[n_pulses, n_bones, 3, 4]}: the bone matrices of every pulse (motion.apply_skin's arithmetic);
    `transforms`  None, or float[n_pulses, n_shapes, 3, 4] as in render_motion_sweep, applied on top.

    The scene is built once and the skins attached before it is cloned; the pulses are split into `n_streams` contiguous
    groups, one per handle and stream, each ONE skin batch (bf_render_skin_batch_device).  per_pulse=True is the reference
    path: the pulses rotate over the handles, one bf_scene_pose_skin (+ one bf_scene_transform_meshes) and one render per
    pulse; per-path results are the same.  rebuild_every, classes and recompute_normals (the normals of the POSED surface in
    place of the blended rest normals) as in render_deform_sweep.  dual_quaternion=(shapes...): those skinned meshes are blended
    as unit dual quaternions (Scene.set_skin_mode, motion.apply_skin_dq; their bones must be rigid), which keeps the volume of a
    twisting joint, where by default they are blended linearly.  velocities={shape: dt} with classes=(bins, twists) as in
    render_motion_sweep (one handle and stream then, n_streams ignored).  Returns the cube
    float32[n_pulses, f_bins * t_bins, 3] of (I, Q, W), or float32[n_pulses, n_classes, f_bins * t_bins, 3] with classes."""
    every = _every(rebuild_every)
    n, shapes, tabs = capi.skin_tables(bones)
    skins = {int(k): v for k, v in skins.items()}
    if set(skins) != set(int(k) for k in shapes):
        raise ValueError(f"skins for shapes {sorted(skins)}, bones for shapes {sorted(int(k) for k in shapes)}")
    _meshes_of(sd, shapes)
    xf = _transforms(transforms, n)

    def prepare(first, dev):
        for sh, tab in zip(shapes, tabs):
            rest, rest_n = _rest_pose(sd, sh)
            index, weight = skins[int(sh)]
            first.set_skin(int(sh), tab.shape[1], rest, index, weight, rest_normals=rest_n)
        _dual_quaternion(first, dual_quaternion, set(skins))

    def pose(h, k, stream):
        for sh, tab in zip(shapes, tabs):
            h.pose_skin(int(sh), tab[k], stream=stream)

    def batch(h, lp, c0, c1, cube_ptr, stream):
        h.render_skin_batch_device(lp, {int(sh): tab[c0:c1] for sh, tab in zip(shapes, tabs)}, cube_ptr,
                                   transforms=None if xf is None else xf[c0:c1], stream=stream)

    return _version_sweep(sd, launch, n, xf, n_streams, per_pulse, every, classes, recompute_normals, lib, device, prepare, pose, batch, velocities)


def render_morph_sweep(sd, launch, morphs, weights, skins=None, bones=None, transforms=None, n_streams=2, per_pulse=False, rebuild_every=None,
                       classes=None, recompute_normals=(), lib=None, device=None, dual_quaternion=None, velocities=None):
    """Coherent pulse sweep in which meshes are moved by MORPH TARGETS (blend shapes), a few weights per pulse: the
    counterpart of render_skin_sweep for surfaces that bones describe badly, a breathing chest wall or a panel vibrating in a
    few modes.  A mesh may be skinned behind its morph.

    `morphs`      {shape: delta_positions float32[n_targets, n_vertices, 3]} or {shape: (delta_positions, delta_normals)}: the
                  targets of every morphed mesh; its rest shape is the mesh as `sd` describes it (positions, and vertex
                  normals if it has any);
    `weights`     {shape: float32[n_pulses, n_targets]}: the weights of every pulse (motion.apply_morph's arithmetic);
    `skins`       None, or {shape: (index, weight)} as in render_skin_sweep for some of the morphed meshes, with
    `bones`       {shape: float32[n_pulses, n_bones, 3, 4]} for exactly those;
    `transforms`  None, or float[n_pulses, n_shapes, 3, 4] as in render_motion_sweep, applied on top.

    The scene is built once and the morphs and skins attached before it is cloned; the pulses are split into `n_streams`
    contiguous groups, one per handle and stream, each ONE morph batch (bf_render_morph_batch_device).  per_pulse=True is the
    reference path: the pulses rotate over the handles, one bf_scene_pose_morph (+ one bf_scene_transform_meshes) and one
    render per pulse; per-path results are the same.  rebuild_every, classes, recompute_normals and dual_quaternion (for skinned
    meshes) as in render_skin_sweep, velocities={shape: dt} as in render_motion_sweep (one handle and stream then).
    Returns the cube float32[n_pulses, f_bins * t_bins, 3] of (I, Q, W), or float32[n_pulses, n_classes, f_bins * t_bins, 3]
    with classes."""
    every = _every(rebuild_every)
    n, shapes, tabs = capi.morph_tables(weights)
    morphs = {int(k): (v if isinstance(v, tuple) else (v, None)) for k, v in morphs.items()}
    if set(morphs) != set(int(k) for k in shapes):
        raise ValueError(f"morphs for shapes {sorted(morphs)}, weights for shapes {sorted(int(k) for k in shapes)}")
    skins = {int(k): v for k, v in (skins or {}).items()}
    btabs = {}
    if skins or bones:
        nb, bshapes, bt = capi.skin_tables(bones or {})
        btabs = {int(k): t for k, t in zip(bshapes, bt)}
        if set(skins) != set(btabs) or not set(skins) <= set(morphs) or nb != n:
            raise ValueError(f"skins for shapes {sorted(skins)}, bones for shapes {sorted(btabs)} over {nb} pulses, morphs for shapes "
                             f"{sorted(morphs)} over {n}")
    _meshes_of(sd, shapes)
    xf = _transforms(transforms, n)

    def prepare(first, dev):
        for sh, tab in zip(shapes, tabs):
            rest, rest_n = _rest_pose(sd, sh)
            dp, dn = morphs[int(sh)]
            first.set_morph(int(sh), tab.shape[1], rest, dp, rest_normals=rest_n, delta_normals=dn)
            if int(sh) in skins:
                index, weight = skins[int(sh)]
                first.set_skin(int(sh), btabs[int(sh)].shape[1], rest, index, weight, rest_normals=rest_n)
        _dual_quaternion(first, dual_quaternion, set(skins))

    def pose(h, k, stream):
        for sh, tab in zip(shapes, tabs):
            b = btabs.get(int(sh))
            h.pose_morph(int(sh), tab[k], bones=None if b is None else b[k], stream=stream)

    def batch(h, lp, c0, c1, cube_ptr, stream):
        h.render_morph_batch_device(lp, {int(sh): tab[c0:c1] for sh, tab in zip(shapes, tabs)}, cube_ptr,
                                    bones={k: t[c0:c1] for k, t in btabs.items()} or None,
                                    transforms=None if xf is None else xf[c0:c1], stream=stream)

    return _version_sweep(sd, launch, n, xf, n_streams, per_pulse, every, classes, recompute_normals, lib, device, prepare, pose, batch, velocities)


def range_doppler(cube, window=True):
    """Slow-time FFT of a pulse-sweep cube: complex64[n_doppler, cells], zero Doppler at row 0 (numpy.fft order)."""
    z = cube[:, :, 0].astype(np.complex64) + 1j * cube[:, :, 1].astype(np.complex64)
    if window:
        z = z * np.hanning(z.shape[0])[:, None].astype(np.float32)
    return np.fft.fft(z, axis=0)
