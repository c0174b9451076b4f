"""Developer A/B: renders with and without returns by target class (BF_FLAG_CLASSES, 5 classes) on the full-size bench scenes,
interleaved run by run, with the per-kernel times of BF_FLAG_STATS.

    python tools/class_ab.py [--runs 5] [--steps 6] [--configs c4,c2] [--arrival] [--range-rate] [--vertex-velocity]

c4 : one C4 shard (bus + car + motorbike, 4096 range bins, 2^19 paths) per render.  5 classes x 4101 floats = 20505 >
     kMaxLdsHist: the classed render takes global atomics BY SIZE, the plain one privatises its histogram in LDS.
c2 : C2 (bus, 256 range bins).  5 x 261 floats: both renders privatise in LDS.
c4full : the whole of C4 (2^22 paths) per render, otherwise c4.
Classes do not roll, so every render is a stand-alone one on one handle (bench.py's "iso" probe), timed by the library
(bf_stats: whole render, wf_shade, wf_trace, tail).  Four modes per config, so that the cost of the flag can be told from what
it brings along:
    lean        the plain render as bench.py runs it (lean kernels, base channels in registers)
    general     the plain render on a handle created under BF_LEAN=0 (the general kernels: what the class variants are built from)
    general_ga  ... with BF_FLAG_GLOBAL_ATOMICS (what a classed C4 render is forced into by size)
    classed     BF_FLAG_CLASSES, ground / bus / car / motorbike / miss
    arrival     (--arrival) BF_FLAG_CLASSES under an arrival table of as many classes (Scene.set_arrival_classes: 4 x 1 azimuth bins
                over the camera's field of view and the class outside), on a handle of its own: the cost of the class from the
                primary ray's direction against the class from the first intersection, at equal n_classes
    range_rate  (--range-rate) BF_FLAG_CLASSES under a range-rate table of as many classes (Scene.set_range_rate_classes: 3 bins over
                [-24, 0) m/s, the class outside and the miss class; the radar at 6 m/s along +x, aperture and ground at rest, mesh k closing at
                4 (k + 1) m/s and yawing at 0.5 rad/s about the origin), on a handle of its own: the cost of the class from the first
                intersection's range rate (a per-lane row of twelve words and some thirty fp32 operations) against one table word
    rr_vertex, rr_difference  (--vertex-velocity, with --range-rate) the same table and twists on two more handles whose meshes are in
                BF_VELOCITY_VERTEX (an explicit field: every mesh spinning at 0.3 rad/s about its centroid's vertical) and in
                BF_VELOCITY_DIFFERENCE (dt = 1/64 s, every mesh stepped 1 cm along -x by one bf_scene_transform_meshes and back, so
                the geometry rendered is the description's and the field that of the step back): the cost of the three velocity
                rows per hit and the interpolation against the twist alone (range_rate: BF_VELOCITY_TWIST)
Prints one line per config and mode: medians over runs x steps of kernel_ms, shade_ms, trace_ms, tail_ms, the spread of kernel_ms
and kernel_ms relative to `lean` and to `classed`."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--configs", default="c4,c2")
    ap.add_argument("--arrival", action="store_true")
    ap.add_argument("--range-rate", action="store_true")
    ap.add_argument("--vertex-velocity", action="store_true")
    args = ap.parse_args()
    import numpy as np
    import torch
    from beifong_amd import capi, motion, scenes
    import bench

    dev = torch.device("cuda", 0)
    lib = capi.load_library()
    CLS, GA, STATS = capi.BF_FLAG_CLASSES, capi.BF_FLAG_GLOBAL_ATOMICS, capi.BF_FLAG_STATS

    class A:       # the bench arguments Workload reads
        paths = tris = cpu_paths = streams = 0
        pulses = 64
        scaling = "weak"
        rolling = 0

    def run_config(name, cfg):
        a = A()
        a.config = cfg
        w = bench.Workload(a, 0, 1, capi, scenes)
        n_shapes = len(w.sd.shapes)
        # aperture and ground together, one class per mesh (C2 has one: two classes stay empty), the paths that leave the scene
        shape_class = [0, 0] + [min(1 + k, 3) for k in range(n_shapes - 2)]
        lean = capi.Scene(w.sd, lib)
        lean.set_classes(shape_class, 5, 4)
        os.environ["BF_LEAN"] = "0"
        general = capi.Scene(w.sd, lib)          # the tunables are read when a scene is created
        del os.environ["BF_LEAN"]
        modes = {"lean": (lean, 0), "general": (general, 0), "general_ga": (general, GA), "classed": (lean, CLS)}
        handles = [lean, general]
        if args.arrival:
            by_angle = capi.Scene(w.sd, lib)
            assert by_angle.set_arrival_classes(capi.arrival_bins_for(w.sd, 4, 1, (-0.3, 0.3, -2.0, 2.0))) == 5
            modes["arrival"] = (by_angle, CLS)
            handles.append(by_angle)
        if args.range_rate:
            by_rate = capi.Scene(w.sd, lib)
            # the aperture and the ground at rest, as shape_class above has them; mesh k = shape 2 + k
            twists = [motion.twist()] * 2 + [motion.twist(lin=(-4.0 * (k + 1), 0.0, 0.0), ang=(0.0, 0.0, 0.5)) for k in range(n_shapes - 2)]
            assert by_rate.set_range_rate_classes(capi.range_rate_bins((-24.0, 0.0), 3, sensor_lin=(6.0, 0.0, 0.0)), twists) == 5
            modes["range_rate"] = (by_rate, CLS)
            handles.append(by_rate)
            if args.vertex_velocity:
                bins = capi.range_rate_bins((-24.0, 0.0), 3, sensor_lin=(6.0, 0.0, 0.0))
                meshes = [k for k, s in enumerate(w.sd.shapes) if s.type == capi.BF_SHAPE_MESH]
                by_vertex = capi.Scene(w.sd, lib)
                assert by_vertex.set_range_rate_classes(bins, twists) == 5
                for k in meshes:
                    s = w.sd.shapes[k]
                    p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).astype(np.float32)
                    by_vertex.set_velocity_mode(k, capi.BF_VELOCITY_VERTEX)
                    by_vertex.set_vertex_velocities(k, np.cross(np.float32([0.0, 0.0, 0.3]), p - p.mean(0, dtype=np.float32)).astype(np.float32))
                by_diff = capi.Scene(w.sd, lib)
                assert by_diff.set_range_rate_classes(bins, twists) == 5
                for k in meshes:
                    by_diff.set_velocity_mode(k, capi.BF_VELOCITY_DIFFERENCE, 1.0 / 64.0)
                xf = np.tile(motion.rigid(), (n_shapes, 1, 1)).astype(np.float32)
                for k in meshes:
                    xf[k] = motion.rigid(t=(-0.01, 0.0, 0.0))
                by_diff.transform_meshes(xf)
                by_diff.transform_meshes(np.tile(motion.rigid(), (n_shapes, 1, 1)).astype(np.float32))
                modes["rr_vertex"], modes["rr_difference"] = (by_vertex, CLS), (by_diff, CLS)
                handles += [by_vertex, by_diff]
        hist = torch.zeros(lean.channels(w.launch(0, CLS)), dtype=torch.float32, device=dev)
        keys = ("kernel_ms", "shade_ms", "trace_ms", "tail_ms")
        ms = {m: {k: [] for k in keys} for m in modes}
        variant = {}

        def region(mode, keep):
            g, flags = modes[mode]
            for i in range(args.steps):
                hist.zero_()
                torch.cuda.synchronize()
                st = g.render_device(w.launch(i, flags | STATS), hist.data_ptr(), want_stats=True)
                variant[mode] = st.kernel_variant
                if keep:
                    for k in keys:
                        ms[mode][k].append(getattr(st, k))

        for m in modes:                          # warm-up (pools, launch plans)
            region(m, False)
        order = list(modes)
        for r in range(args.runs):
            for m in (order if r % 2 == 0 else order[::-1]):
                region(m, True)
        base, shape_form = np.median(ms["lean"]["kernel_ms"]), np.median(ms["classed"]["kernel_ms"])
        lp = w.launch(0, CLS)
        print(f"{name}: {int(lp.n_paths)} paths, {lean.channels(w.launch(0))} floats plain, {lean.channels(lp)} classed", flush=True)
        for m in modes:
            k = ms[m]["kernel_ms"]
            print(f"  {m:11s} variant {variant[m]:2d}  kernel {np.median(k):8.3f} ms ({min(k):.3f}..{max(k):.3f})  shade {np.median(ms[m]['shade_ms']):8.3f}"
                  f"  trace {np.median(ms[m]['trace_ms']):8.3f}  tail {np.median(ms[m]['tail_ms']):8.3f}  kernel / lean {np.median(k) / base:.3f}  / classed {np.median(k) / shape_form:.3f}", flush=True)
        for g in handles:
            g.close()

    for cfg in args.configs.split(","):
        if cfg == "c4":
            run_config(cfg, "c4shard")
        elif cfg == "c2":
            run_config(cfg, "c2")
        elif cfg == "c4full":
            run_config(cfg, "c4")
        else:
            raise SystemExit(f"unknown config {cfg}")


if __name__ == "__main__":
    main()
