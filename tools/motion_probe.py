"""Cost of per-mesh rigid motion (bf_scene_transform_meshes) on the full-size C4 scene (scenes.multi_mesh_radar,
~1.5 M triangles).

    python tools/motion_probe.py [--reps 5] [--paths 4194304]

Prints one JSON line:
  create_ms          wall time of capi.Scene(sd) (host binned-SAH build + upload): what a rebuild per frame costs
  first_transform_ms wall time of the handle's first transform (reads the tree topology and the mesh boxes back once)
  refit_ms           device time of one transform (triangle transform + one refit launch per tree level + re-quantisation),
                     hip events around the call on its stream, median over --reps
  trace_ms_*         wf_trace time (bf_stats.trace_ms) of one C4 render, median over --reps: as created, with the car turned
                     by 30 and by 90 degrees about its centre (refitted tree), and a scene rebuilt in the 90 degree pose
Run the refit timing under `rocprofv3 --kernel-trace --stats -- python tools/motion_probe.py` for the per-kernel split."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", type=int, default=4096 << 10)
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    import numpy as np
    import torch
    from beifong_amd import capi, motion, scenes

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    sd, lp = scenes.multi_mesh_radar(n_paths=args.paths, scale=args.scale)
    meshes = [k for k, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH]
    car = meshes[1]
    s = sd.shapes[car]
    p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).astype(np.float64)
    centre = 0.5 * (p.min(0) + p.max(0))

    def pose(deg):
        xf = np.tile(motion.rigid(), (len(sd.shapes), 1, 1))
        xf[car] = motion.about(motion.rotation([0, 0, 1], deg), centre)
        return xf

    out = {"n_triangles": 0}
    t0 = time.perf_counter()
    g = capi.Scene(sd)
    out["create_ms"] = (time.perf_counter() - t0) * 1e3
    out["n_triangles"] = int(g.info().n_triangles)

    def trace_ms(h):
        lst = []
        for _ in range(args.reps):
            _, _, st = h.render(lp)
            lst.append(st.trace_ms)
        return float(np.median(lst))

    g.render(lp)                                   # warm-up
    out["trace_ms_created"] = trace_ms(g)
    stream = torch.cuda.Stream(dev)
    t0 = time.perf_counter()
    g.transform_meshes(pose(30.0), stream=stream.cuda_stream)
    stream.synchronize()
    out["first_transform_ms"] = (time.perf_counter() - t0) * 1e3
    refit = []
    for i in range(args.reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        g.transform_meshes(pose(30.0 + 0.5 * (i % 2)), stream=stream.cuda_stream)
        b.record(stream)
        b.synchronize()
        refit.append(a.elapsed_time(b))
    out["refit_ms"] = float(np.median(refit))
    out["refit_ms_all"] = [round(x, 4) for x in refit]
    g.transform_meshes(pose(30.0), stream=stream.cuda_stream)
    stream.synchronize()
    out["trace_ms_car30"] = trace_ms(g)
    g.transform_meshes(pose(90.0), stream=stream.cuda_stream)
    stream.synchronize()
    out["trace_ms_car90"] = trace_ms(g)
    t0 = time.perf_counter()
    fresh = capi.Scene(motion.moved_description(sd, pose(90.0)))
    out["create_moved_ms"] = (time.perf_counter() - t0) * 1e3
    fresh.render(lp)
    out["trace_ms_car90_rebuilt"] = trace_ms(fresh)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}))


if __name__ == "__main__":
    main()
