"""Cost and effect of the device BVH rebuild (bf_scene_rebuild_bvh) on the full-size C4 scene
(scenes.multi_mesh_radar, ~1.5 M triangles).

    python tools/rebuild_probe.py [--reps 5] [--paths 1048576]

For three changes of the car mesh — the twist deformation, the ripple, the car turned 30 degrees — prints one JSON line each:
  rebuild_ms / rebuild_wall_ms   one rebuild_bvh: hip events around the call on its stream, and the wall clock of the call,
                                 median over --reps after a warm-up
  create_ms                      wall time of capi.Scene(sd') of the same vertices (host binned-SAH build + upload)
  trace_ms_*, nodes_per_ray_*, tris_per_ray_*
                                 bf_stats.trace_ms (median over --reps) and, from one BF_FLAG_STATS render of the same seed, the
                                 nodes visited and triangles tested per traced ray, for three trees of the same vertices:
                                 refit (re-fitted), device (rebuilt on the device), host (created fresh)
The deformations are the test suite's (tests/test_gpu_deform.py: deform), imported from the repository root, so that the
probe measures exactly the cases the tests hold to the oracle.
Run it under `rocprofv3 --kernel-trace --stats -- python tools/rebuild_probe.py` for the builder's per-kernel split."""
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
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--cases", default="twist,ripple,car30")
    args = ap.parse_args()
    import numpy as np
    import torch
    from beifong_amd import capi, motion, scenes
    from tests.test_gpu_deform import deform

    dev = torch.device("cuda", 0)
    torch.zeros(1, device=dev)
    sd, lp = scenes.multi_mesh_radar(n_paths=args.paths, scale=args.scale)
    meshes = [k for k, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH]
    car = max(meshes, key=lambda m: sd.shapes[m].n_faces)
    s = sd.shapes[car]
    p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).astype(np.float64)
    centre = 0.5 * (p.min(0) + p.max(0))
    stream = torch.cuda.Stream(dev)
    lp_stats = capi.make_launch(lp.mode, int(lp.n_paths), seed=lp.seed, bins=lp.bins, bins_y=lp.bins_y, bin_width=lp.bin_width,
                                color_mode=lp.color_mode, max_depth=lp.max_depth, rr_depth=lp.rr_depth, time_c=lp.time_c,
                                phase_bins=lp.phase_bins, flags=lp.flags | capi.BF_FLAG_STATS)

    def measure(h, tag, out):
        h.render(lp)
        out[f"trace_ms_{tag}"] = float(np.median([h.render(lp)[2].trace_ms for _ in range(args.reps)]))
        st = h.render(lp_stats)[2]
        rays = max(1, int(st.n_rays_closest + st.n_rays_shadow))
        out[f"nodes_per_ray_{tag}"] = st.n_nodes_visited / rays
        out[f"tris_per_ray_{tag}"] = st.n_tris_tested / rays

    for case in args.cases.split(","):
        out = {"case": case}
        g = capi.Scene(sd)
        out["n_triangles"] = int(g.info().n_triangles)
        if case == "car30":
            xf = np.tile(motion.rigid(), (len(sd.shapes), 1, 1))
            xf[car] = motion.about(motion.rotation([0, 0, 1], 30.0), centre)
            g.transform_meshes(xf)
            new_sd = motion.moved_description(sd, xf)
        else:
            v, n = deform(sd, car, case)
            g.update_vertices(car, v, n)
            new_sd = motion.deformed_description(sd, {car: (v, n)})
        measure(g, "refit", out)
        i0 = g.info()
        ev, wall = [], []
        for i in range(args.reps + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            t0 = time.perf_counter()
            g.rebuild_bvh(stream=stream.cuda_stream)
            wall.append((time.perf_counter() - t0) * 1e3)
            b.record(stream)
            b.synchronize()
            ev.append(a.elapsed_time(b))
        out["rebuild_ms"] = float(np.median(ev[1:]))
        out["rebuild_wall_ms"] = float(np.median(wall[1:]))
        out["rebuild_wall_ms_all"] = [round(x, 3) for x in wall]
        i1 = g.info()
        out["nodes_refit_device"] = [int(i0.n_bvh_nodes), int(i1.n_bvh_nodes)]
        out["depth_refit_device"] = [int(i0.bvh_depth), int(i1.bvh_depth)]
        measure(g, "device", out)
        t0 = time.perf_counter()
        fresh = capi.Scene(new_sd)
        out["create_ms"] = (time.perf_counter() - t0) * 1e3
        out["nodes_host"] = int(fresh.info().n_bvh_nodes)
        measure(fresh, "host", out)
        out["nodes_per_ray_device_over_host"] = out["nodes_per_ray_device"] / out["nodes_per_ray_host"]
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in out.items()}), flush=True)
        g.close()
        fresh.close()


if __name__ == "__main__":
    main()
