"""Morph poses against what they replace, measured in one run with the variants interleaved rep by rep, medians and
ranges over the reps:

    python tools/morph_ab.py [--reps 5] [--paths 262144] [--pulses 64] [--targets 8] [--streams 2]

C4's multi-mesh scene (1.49 M triangles) with the car morphed: `--targets` targets, each a smooth bulge of the body around one
station along its long axis (neighbouring bulges overlap), the weights a few sinusoids over the sweep.  Three ways to render the
pulses:

  morph_batches    sweep.render_morph_sweep: the pulses' weights are all that is uploaded;
  deform_batches   sweep.render_deform_sweep fed with the vertices motion.apply_morph computes on the host (what a user had to do
                   before; the host morph itself is timed once and printed apart: it is numpy, not the library);
  per_pulse        sweep.render_morph_sweep(per_pulse=True): one bf_scene_pose_morph and one render per pulse.

and the cost of one pose on the device: HIP events around bf_scene_pose_morph against bf_scene_update_vertices_device of the same
vertices; their difference is bf_morph_vertices_kernel and the upload of its weights (`rocprofv3 --kernel-trace --stats -- python
tools/morph_ab.py --reps 1` gives the kernel alone)."""
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


def car_targets(v, n_targets, amplitude=0.05, reach=0.75):
    """float32[n_targets, nv, 3]: target k pushes the vertices within reach * spacing of station k along x away from the body's
    axis (the line through its centre along x) by amplitude (1 - (a / h)^2)^2, as meshgen.bar_swell_targets does for the bar"""
    lo, hi = float(v[:, 0].min()), float(v[:, 0].max())
    c = 0.5 * (v.min(0) + v.max(0)).astype(np.float64)
    radial = (v.astype(np.float64) - c) * [0.0, 1.0, 1.0]
    r = np.linalg.norm(radial, axis=1)
    unit = np.where(r[:, None] > 0.0, radial / np.maximum(r, 1e-300)[:, None], 0.0)
    spacing = (hi - lo) / n_targets
    h = reach * spacing
    out = np.zeros((n_targets, len(v), 3), np.float32)
    for k in range(n_targets):
        a = np.abs(v[:, 0].astype(np.float64) - (lo + (k + 0.5) * spacing))
        out[k] = (unit * (amplitude * np.where(a < h, (1.0 - (a / h) ** 2) ** 2, 0.0))[:, None]).astype(np.float32)
    return out


def breathe(n_targets, n_pulses):
    """float32[n_pulses, n_targets]: weight k = sin(2 pi (pulse / 16 + k / 5))"""
    p, k = np.arange(n_pulses)[:, None], np.arange(n_targets)[None]
    return np.ascontiguousarray(np.sin(2.0 * np.pi * (p / 16.0 + k / 5.0)).astype(np.float32))


def spread(x):
    return {"median_ms": float(np.median(x)), "min_max_ms": [float(min(x)), float(max(x))]}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", type=int, default=1 << 18)
    ap.add_argument("--pulses", type=int, default=64)
    ap.add_argument("--targets", type=int, default=8)
    ap.add_argument("--streams", type=int, default=2)
    a = ap.parse_args()
    sd, lp = scenes.multi_mesh_radar(n_paths=a.paths)
    car = max((k for k, s in enumerate(sd.shapes) if s.type == MESH), key=lambda k: sd.shapes[k].n_vertices)
    s = sd.shapes[car]
    rest = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()
    dp = car_targets(rest, a.targets)
    weights = breathe(a.targets, a.pulses)
    t0 = time.perf_counter()
    pos = np.ascontiguousarray(np.stack([motion.apply_morph(rest, None, dp, None, weights[p])[0] for p in range(a.pulses)]))
    host_morph_ms = 1e3 * (time.perf_counter() - t0)
    morphs = {car: dp}
    runs = {"morph_batches": lambda: sweep.render_morph_sweep(sd, lp, morphs, {car: weights}, n_streams=a.streams),
            "deform_batches": lambda: sweep.render_deform_sweep(sd, lp, {car: pos}, n_streams=a.streams),
            "per_pulse": lambda: sweep.render_morph_sweep(sd, lp, morphs, {car: weights}, n_streams=a.streams, per_pulse=True)}
    cubes = {k: f() for k, f in runs.items()}      # warm-up: pools, arenas, launch plans; and the three agree on what they rendered
    ref = cubes["morph_batches"]
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
    g.set_morph(car, a.targets, rest, dp)
    dv = torch.from_numpy(pos[1]).cuda()
    bound = float(np.abs(pos).max())
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_pose, t_upd = [], []
    for r in range(a.reps + 2):
        ev[0].record()
        g.pose_morph(car, weights[r % a.pulses])
        ev[1].record()
        g.sync()
        t_pose.append(ev[0].elapsed_time(ev[1]))
        ev[0].record()
        g.update_vertices_device(car, dv.data_ptr(), None, bound)
        ev[1].record()
        g.sync()
        t_upd.append(ev[0].elapsed_time(ev[1]))
    t_pose, t_upd = t_pose[2:], t_upd[2:]
    out = {"scene": "C4", "triangles": int(g.info().n_triangles), "morphed_vertices": int(len(rest)), "targets": a.targets, "pulses": a.pulses,
           "paths": a.paths, "streams": a.streams, "reps": a.reps, "host_morph_ms": host_morph_ms,
           "upload_bytes": {"morph_batches": int(weights.nbytes), "deform_batches": int(pos.nbytes)}, "morph_block_bytes": int(rest.nbytes + dp.nbytes)}
    for k, x in t.items():
        out[k] = spread(x)
    out["pose_morph"] = spread(t_pose)
    out["update_vertices_device"] = spread(t_upd)
    out["morph_kernel_and_weights_ms"] = float(np.median(t_pose) - np.median(t_upd))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
