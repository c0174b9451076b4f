"""Vertex updates against what they replace, measured in one run with the variants interleaved rep by rep and
medians over the reps:

    python tools/deform_ab.py [--reps 7] [--paths 1048576] [--pulses 64] [--part update|sweep|loose|all]

  update  C4's multi-mesh scene (1.49 M triangles), all vertices of the car moving: one bf_scene_update_vertices_device (HIP
          events around the call) against one bf_scene_transform_meshes on the same handle against bf_scene_create of the scene
          (wall clock: it is host work).  The per-kernel split comes from `rocprofv3 --kernel-trace --stats -- python
          tools/deform_ab.py --part update`.
  sweep   the motion-batch workload (tools/motion_batch_ab.py: bus + car, receive IQ, pulses x paths on 2 streams) with the car
          deforming: deform batches against per_pulse=True against the rigid motion batch of the same poses.
  loose   wf_trace per render (bf_stats.trace_ms of a stats render) on the tree re-fitted after the twist deformation of
          tests/test_gpu_deform.py against a scene created from the same vertices: what a loosened tree costs."""
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


def _verts(sd, k):
    s = sd.shapes[k]
    return np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()


def twist(p):
    """the non-uniform scale + twist of tests/test_gpu_deform.py"""
    p = p.astype(np.float64)
    c = 0.5 * (p.min(0) + p.max(0))
    d = (p - c) * np.array([1.5, 0.7, 1.2])
    ang = 1.1 * (p[:, 2] - p[:, 2].min())
    cs, sn = np.cos(ang), np.sin(ang)
    return np.ascontiguousarray(np.stack([cs * d[:, 0] - sn * d[:, 1], sn * d[:, 0] + cs * d[:, 1], d[:, 2]], 1) + c, dtype=np.float32)


def med(x):
    return float(np.median(x))


def part_update(reps):
    import torch
    sd, lp = scenes.multi_mesh_radar(n_paths=1 << 16)
    meshes = [k for k, s in enumerate(sd.shapes) if s.type == MESH]
    car = max(meshes, key=lambda k: sd.shapes[k].n_vertices)
    v = _verts(sd, car)
    frames = [torch.from_numpy((v + np.float32(0.01 * (i + 1)) * np.sin(v[:, ::-1] * 7.0).astype(np.float32))).cuda() for i in range(2)]
    bound = float(max(f.abs().max() for f in frames))
    xf = {car: motion.rigid(t=(0.1, 0.0, 0.0))}
    g = capi.Scene(sd)
    g.update_vertices_device(car, frames[0].data_ptr(), None, bound)
    g.transform_meshes(xf)
    g.sync()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t_upd, t_xf, t_new = [], [], []
    for r in range(reps):
        ev[0].record()
        g.update_vertices_device(car, frames[r % 2].data_ptr(), None, bound)
        ev[1].record()
        g.sync()
        t_upd.append(ev[0].elapsed_time(ev[1]))
        ev[0].record()
        g.transform_meshes(xf)
        ev[1].record()
        g.sync()
        t_xf.append(ev[0].elapsed_time(ev[1]))
        t0 = time.perf_counter()
        h = capi.Scene(sd)
        torch.cuda.synchronize()
        t_new.append(1e3 * (time.perf_counter() - t0))
        h.close()
    return {"triangles": int(g.info().n_triangles), "vertices_moved": int(v.shape[0]), "update_vertices_device_ms": med(t_upd),
            "transform_meshes_ms": med(t_xf), "scene_create_ms": med(t_new), "reps": reps}


def part_sweep(reps, n_paths, n_pulses, n_streams):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import motion_batch_ab as mb
    sd, lp = mb.build(n_paths)
    xf, _ = mb.poses(sd, n_pulses)
    car = [k for k, s in enumerate(sd.shapes) if s.type == MESH][-1]
    v = _verts(sd, car)
    w = np.sin(2.0 * np.pi * np.arange(n_pulses) / 16.0)
    pos = np.ascontiguousarray((v[None] + (0.01 * w)[:, None, None] * np.sin(v[None, :, ::-1] * 5.0)).astype(np.float32))
    runs = {"deform_batches": lambda: sweep.render_deform_sweep(sd, lp, {car: pos}, transforms=xf, n_streams=n_streams),
            "per_pulse": lambda: sweep.render_deform_sweep(sd, lp, {car: pos}, transforms=xf, n_streams=n_streams, per_pulse=True),
            "rigid_motion_batches": lambda: sweep.render_motion_sweep(sd, lp, xf, n_streams=n_streams)}
    for f in runs.values():
        f()                             # warm-up: pools, arenas, launch plans
    t = {k: [] for k in runs}
    t["scene_build"] = []               # what every call above does first on the host: the constant all three share
    for r in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        first = capi.Scene(sd)
        others = [first.clone() for _ in range(n_streams - 1)]
        torch.cuda.synchronize()
        t["scene_build"].append(1e3 * (time.perf_counter() - t0))
        for h in others + [first]:
            h.close()
        for k, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            t[k].append(1e3 * (time.perf_counter() - t0))
    # (each call builds its scene: the same host work in all three; scene_build_ms is that constant, measured in the same reps)
    out = {"pulses": n_pulses, "paths": n_paths, "streams": n_streams, "reps": reps}
    for k, x in t.items():
        out[k + "_ms"] = med(x)
        out[k + "_min_max_ms"] = [float(min(x)), float(max(x))]
    return out


def part_loose(reps):
    sd, lp = scenes.multi_mesh_radar(n_paths=1 << 20)
    meshes = [k for k, s in enumerate(sd.shapes) if s.type == MESH]
    car = max(meshes, key=lambda k: sd.shapes[k].n_vertices)
    v = twist(_verts(sd, car))
    a = capi.Scene(sd)
    a.update_vertices(car, v)
    b = capi.Scene(motion.deformed_description(sd, {car: v}))
    ta, tb = [], []
    for r in range(reps + 2):
        sa = a.render(lp)[2]
        sb = b.render(lp)[2]
        if r >= 2:
            ta.append(sa.trace_ms)
            tb.append(sb.trace_ms)
    return {"refitted_trace_ms": med(ta), "rebuilt_trace_ms": med(tb), "ratio": med(ta) / max(med(tb), 1e-9), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--pulses", type=int, default=64)
    ap.add_argument("--streams", type=int, default=2)
    ap.add_argument("--part", default="all", choices=["update", "sweep", "loose", "all"])
    a = ap.parse_args()
    out = {}
    if a.part in ("update", "all"):
        out["update"] = part_update(a.reps)
    if a.part in ("loose", "all"):
        out["loose"] = part_loose(a.reps)
    if a.part in ("sweep", "all"):
        out["sweep"] = part_sweep(a.reps, a.paths, a.pulses, a.streams)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
