"""What the dual-quaternion blend costs against the linear one, measured in one process with the two modes
interleaved pose by pose:

    python tools/skin_mode_ab.py [--reps 30] [--bones 32] [--tris 1000000]

C3's scene (scenes.car_radar: a car-body shell with vertex normals over a ground plane) with the car skinned to `--bones` bones
along its long axis as tools/skin_ab.py skins C4's car, each joint turned about the vertical by a few degrees.  One handle; a pose
is bf_scene_pose_skin between two HIP events on the null stream, so a figure holds the upload of the bone table, the skin kernel, the
gather into triangle rows and the refit of both trees; only the table (8 floats per bone against 12, and its conversion on the host,
which the events do not see) and the skin kernel differ between the modes.  The yardstick is the linear mode of the same build.
Prints one JSON line: per mode the median and the range over the reps after two warm-up poses each, and the wall time of the call
(host side included) the same way."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import beifong_amd

beifong_amd.configure_runtime()
from beifong_amd import capi, scenes
from tools.skin_ab import car_skin, spread, swing

MODES = {"linear": capi.BF_SKIN_LINEAR, "dual_quaternion": capi.BF_SKIN_DUAL_QUATERNION}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--bones", type=int, default=32)
    ap.add_argument("--tris", type=int, default=1_000_000)
    a = ap.parse_args()
    if a.reps < 20:
        ap.error("--reps: at least 20 poses per mode")
    sd, lp = scenes.car_radar(n_tris=a.tris, n_paths=1 << 16, bins=1024, dr=0.03)
    car = max((k for k, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH), key=lambda k: sd.shapes[k].n_vertices)
    s = sd.shapes[car]
    rest = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).copy()
    rest_n = np.ctypeslib.as_array(s.normals, shape=(s.n_vertices, 3)).copy() if s.normals else None
    index, weight, joints = car_skin(rest, a.bones)
    warm = 2
    bones = swing(joints, a.reps + warm)
    g = capi.Scene(sd)
    g.set_skin(car, a.bones, rest, index, weight, rest_normals=rest_n)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    dev = {k: [] for k in MODES}
    wall = {k: [] for k in MODES}
    for r in range(a.reps + warm):
        for name, mode in (MODES.items() if r % 2 == 0 else reversed(list(MODES.items()))):      # interleaved, the order alternating
            g.set_skin_mode(car, mode)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev[0].record()
            g.pose_skin(car, bones[r])
            ev[1].record()
            g.sync()
            wall[name].append(1e3 * (time.perf_counter() - t0))
            dev[name].append(ev[0].elapsed_time(ev[1]))
    out = {"scene": "C3", "triangles": int(g.info().n_triangles), "skinned_vertices": int(len(rest)), "vertex_normals": rest_n is not None,
           "bones": a.bones, "reps": a.reps, "warm_up": warm}
    for name in MODES:
        out[name] = {"events": spread(dev[name][warm:]), "wall": spread(wall[name][warm:])}
    out["dq_over_linear_events"] = out["dual_quaternion"]["events"]["median_ms"] / out["linear"]["events"]["median_ms"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
