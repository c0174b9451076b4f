"""Skinned poses against what they replace, measured in one run with the variants interleaved rep by rep, medians
and ranges over the reps:

    python tools/skin_ab.py [--reps 5] [--paths 262144] [--pulses 64] [--bones 20] [--streams 2]

C4's multi-mesh scene (1.49 M triangles) with the car skinned: `--bones` bones along its long axis, every vertex blended over the
two nearest, each joint swinging about the vertical by a few degrees over the sweep.  Three ways to render the pulses:

  skin_batches     sweep.render_skin_sweep: the pulses' bone tables are all that is uploaded;
  deform_batches   sweep.render_deform_sweep fed with the vertices motion.apply_skin computes on the host (what a user had to do
                   before; the host skinning itself is timed once and printed apart: it is numpy, not the library);
  per_pulse        sweep.render_skin_sweep(per_pulse=True): one bf_scene_pose_skin and one render per pulse.

and the cost of one pose on the device: HIP events around bf_scene_pose_skin against bf_scene_update_vertices_device of the same
vertices; their difference is bf_skin_vertices_kernel and the upload of its bone table (`rocprofv3 --kernel-trace --stats --
python tools/skin_ab.py --reps 1` gives the kernel alone)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import beifong_amd

beifong_amd.configure_runtime()
from beifong_amd import capi, motion, scenes, sweep

MESH = capi.BF_SHAPE_MESH


def car_skin(v, n_bones, blend=0.25):
    """index, weight, joints of `n_bones` equal segments along x over the mesh's extent, blended as meshgen.jointed_bar blends"""
    lo, hi = float(v[:, 0].min()), float(v[:, 0].max())
    x = np.clip((v[:, 0].astype(np.float64) - lo) / (hi - lo) * n_bones, 0.0, n_bones)
    own = np.clip(np.floor(x), 0, n_bones - 1).astype(np.int64)
    joint = np.clip(np.rint(x), 1, max(1, n_bones - 1))
    other = np.where(joint > own, own + 1, own - 1)
    d = np.abs(x - joint)
    w_own = np.where((n_bones > 1) & (d < blend), 0.5 + 0.5 * d / blend, 1.0)
    index = np.zeros((len(v), 4), np.uint32)
    weight = np.zeros((len(v), 4), np.float32)
    index[:, 0], index[:, 1] = own, np.where(w_own < 1.0, other, 0)
    weight[:, 0] = w_own.astype(np.float32)
    weight[:, 1] = np.float32(1.0) - weight[:, 0]
    c = 0.5 * (v.min(0) + v.max(0)).astype(np.float64)
    joints = np.stack([np.linspace(lo, hi, n_bones + 1), np.full(n_bones + 1, c[1]), np.full(n_bones + 1, c[2])], -1)
    return index, weight, joints


def swing(joints, n_pulses, deg=2.0):
    """float32[n_pulses, n_bones, 3, 4]: a chain in which joint k turns about z by deg sin(2 pi (pulse / 16 + k / 5))"""
    n_bones = len(joints) - 1
    out = np.zeros((n_pulses, n_bones, 3, 4), np.float32)
    for p in range(n_pulses):
        m = np.eye(4)
        for k in range(n_bones):
            if k:
                a = np.eye(4)
                a[:3] = motion.about(motion.rotation([0, 0, 1], deg * np.sin(2.0 * np.pi * (p / 16.0 + k / 5.0))), joints[k]).astype(np.float64)
                m = m @ a
            out[p, k] = m[:3]
    return out


def spread(x):
    return {"median_ms": float(np.median(x)), "min_max_ms": [float(min(x)), float(max(x))]}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", type=int, default=1 << 18)
    ap.add_argument("--pulses", type=int, default=64)
    ap.add_argument("--bones", type=int, default=20)
    ap.add_argument("--streams", type=int, default=2)
    a = ap.parse_args()
    sd, lp = scenes.multi_mesh_radar(n_paths=a.paths)
    car = max((k for k, s in enumerate(sd.shapes) if s.type == MESH), key=lambda k: sd.shapes[k].n_vertices)
    s = sd.shapes[car]
    rest = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()
    index, weight, joints = car_skin(rest, a.bones)
    bones = swing(joints, a.pulses)
    t0 = time.perf_counter()
    pos = np.ascontiguousarray(np.stack([motion.apply_skin(rest, None, index, weight, bones[p])[0] for p in range(a.pulses)]))
    host_skin_ms = 1e3 * (time.perf_counter() - t0)
    skins = {car: (index, weight)}
    runs = {"skin_batches": lambda: sweep.render_skin_sweep(sd, lp, skins, {car: bones}, n_streams=a.streams),
            "deform_batches": lambda: sweep.render_deform_sweep(sd, lp, {car: pos}, n_streams=a.streams),
            "per_pulse": lambda: sweep.render_skin_sweep(sd, lp, skins, {car: bones}, n_streams=a.streams, per_pulse=True)}
    cubes = {k: f() for k, f in runs.items()}      # warm-up: pools, arenas, launch plans; and the three agree on what they rendered
    ref = cubes["skin_batches"]
    for k in ("deform_batches", "per_pulse"):       # the same paths, summed in another order
        assert np.allclose(cubes[k], ref, rtol=1e-3, atol=1e-3 * float(np.abs(ref).max())), k
    t = {k: [] for k in runs}
    for r in range(a.reps):
        for k, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t[k].append(1e3 * (time.perf_counter() - t0))
    # one pose on the device against one device-form vertex update of the same vertices
    g = capi.Scene(sd)
    g.set_skin(car, a.bones, rest, index, weight)
    dv = torch.from_numpy(pos[1]).cuda()
    bound = float(np.abs(pos).max())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_pose, t_upd = [], []
    for r in range(a.reps + 2):
        ev[0].record()
        g.pose_skin(car, bones[r % a.pulses])
        ev[1].record()
        g.sync()
        t_pose.append(ev[0].elapsed_time(ev[1]))
        ev[0].record()
        g.update_vertices_device(car, dv.data_ptr(), None, bound)
        ev[1].record()
        g.sync()
        t_upd.append(ev[0].elapsed_time(ev[1]))
    t_pose, t_upd = t_pose[2:], t_upd[2:]
    out = {"scene": "C4", "triangles": int(g.info().n_triangles), "skinned_vertices": int(len(rest)), "bones": a.bones, "pulses": a.pulses,
           "paths": a.paths, "streams": a.streams, "reps": a.reps, "host_skinning_ms": host_skin_ms,
           "upload_bytes": {"skin_batches": int(bones.nbytes), "deform_batches": int(pos.nbytes)}}
    for k, x in t.items():
        out[k] = spread(x)
    out["pose_skin"] = spread(t_pose)
    out["update_vertices_device"] = spread(t_upd)
    out["skin_kernel_and_table_ms"] = float(np.median(t_pose) - np.median(t_upd))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
