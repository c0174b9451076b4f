"""Recomputed vertex normals against what they replace, measured in one run with the variants interleaved rep by rep,
medians and ranges over the reps:

    python tools/normals_ab.py [--reps 7] [--paths 262144] [--pulses 64] [--bones 20] [--streams 2]

C4's multi-mesh scene (1.49 M triangles) with the car (501 501 vertices) given vertex normals (motion.vertex_normals_f32 of its
placed positions), then deformed:

  recompute        bf_scene_update_vertices_device under BF_NORMALS_RECOMPUTE: positions from a device tensor, no normals;
  given            the same call on a second handle with the normals given from a device tensor (computed on the host, uploaded
                   once, outside the timing): what the gather and the refit cost without the new kernel.  The difference of the two
                   medians is bf_vertex_normals_kernel (`rocprofv3 --kernel-trace --stats -- python tools/normals_ab.py --reps 1`
                   gives the kernel alone);
  host_form        bf_scene_update_vertices with positions and host-computed normals (wall clock to bf_scene_sync: it uploads
                   both arrays), and the host computation (bf_vertex_normals, one thread) timed apart;
  skin sweeps      sweep.render_skin_sweep of --pulses pulses, the car skinned as in tools/skin_ab.py, with and without
                   recompute_normals (without: the skin kernel blends the rest normals)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np

import beifong_amd

beifong_amd.configure_runtime()
from beifong_amd import capi, motion, scenes, sweep
from skin_ab import car_skin, spread, swing

MESH = capi.BF_SHAPE_MESH
f32 = np.float32


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--paths", type=int, default=1 << 18)
    ap.add_argument("--pulses", type=int, default=64)
    ap.add_argument("--bones", type=int, default=20)
    ap.add_argument("--streams", type=int, default=2)
    a = ap.parse_args()
    sd, lp = scenes.multi_mesh_radar(n_paths=a.paths)
    car = max((k for k, s in enumerate(sd.shapes) if s.type == MESH), key=lambda k: sd.shapes[k].n_vertices)
    s = sd.shapes[car]
    rest = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()
    faces = np.ctypeslib.as_array(s.indices, shape=(s.n_faces, 3)).copy()
    rest_n = motion.vertex_normals_f32(rest, faces)
    s.normals = rest_n.ctypes.data_as(C.POINTER(C.c_float))       # C4's car as a smooth-shaded target
    sd._keep.append(rest_n)
    sd.finalize()
    valence = np.bincount(faces.reshape(-1), minlength=len(rest))
    # two deformed frames to alternate between: a ripple along the normals
    frames = [np.ascontiguousarray((rest + f32(0.01 * (i + 1)) * np.sin(rest @ f32([9.0, 5.0, 13.0]))[:, None] * rest_n).astype(f32)) for i in range(2)]
    t0 = time.perf_counter()
    frame_n = [motion.vertex_normals_f32(p, faces) for p in frames]
    host_normals_ms = 1e3 * (time.perf_counter() - t0) / len(frames)
    bound = float(max(np.abs(p).max() for p in frames))
    g, h, u = capi.Scene(sd), capi.Scene(sd), capi.Scene(sd)
    g.set_normal_mode(car, capi.BF_NORMALS_RECOMPUTE)
    dv = [torch.from_numpy(p).cuda() for p in frames]
    dn = [torch.from_numpy(n).cuda() for n in frame_n]
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    t = {"recompute": [], "given": [], "host_form_wall": []}
    for r in range(a.reps + 2):
        i = r % 2
        ev[0].record()
        g.update_vertices_device(car, dv[i].data_ptr(), None, bound)
        ev[1].record()
        g.sync()
        t["recompute"].append(ev[0].elapsed_time(ev[1]))
        ev[0].record()
        h.update_vertices_device(car, dv[i].data_ptr(), dn[i].data_ptr(), bound)
        ev[1].record()
        h.sync()
        t["given"].append(ev[0].elapsed_time(ev[1]))
        t0 = time.perf_counter()
        u.update_vertices(car, frames[i], frame_n[i])
        u.sync()
        t["host_form_wall"].append(1e3 * (time.perf_counter() - t0))
    t = {k: x[2:] for k, x in t.items()}
    # the three handles hold the same rows: the device's normals are the host's, bit for bit
    rows = [x.debug_read_tree(4)[2] for x in (g, h, u)]
    assert np.array_equal(rows[0].view(np.uint32), rows[1].view(np.uint32)) and np.array_equal(rows[0].view(np.uint32), rows[2].view(np.uint32))
    for x in (g, h, u):
        x.close()
    # skin sweeps with and without recomputed normals
    index, weight, joints = car_skin(rest, a.bones)
    bones = swing(joints, a.pulses)
    skins = {car: (index, weight)}
    runs = {"skin_sweep_blended": lambda: sweep.render_skin_sweep(sd, lp, skins, {car: bones}, n_streams=a.streams),
            "skin_sweep_recompute": lambda: sweep.render_skin_sweep(sd, lp, skins, {car: bones}, n_streams=a.streams, recompute_normals=(car,))}
    for f in runs.values():
        f()                                  # warm-up
    ts = {k: [] for k in runs}
    for r in range(max(3, a.reps // 2)):
        for k, f in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            ts[k].append(1e3 * (time.perf_counter() - t0))
    out = {"scene": "C4", "vertices": int(len(rest)), "faces": int(len(faces)), "max_valence": int(valence.max()),
           "mean_valence": float(valence[valence > 0].mean()), "index_bytes": int(48 * len(faces) + 4 * (len(rest) + 1)), "reps": a.reps,
           "pulses": a.pulses, "paths": a.paths, "streams": a.streams, "host_bf_vertex_normals_ms": host_normals_ms}
    for k, x in list(t.items()) + list(ts.items()):
        out[k] = spread(x)
    out["normals_kernel_ms_by_difference"] = float(np.median(t["recompute"]) - np.median(t["given"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
