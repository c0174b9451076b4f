"""Developer A/B: the cost of BF_FLAG_AOV — the plain render against the same render with depth, position and both normals per
pixel — interleaved run by run, with the per-kernel times of BF_FLAG_STATS.

    python tools/aov_ab.py [--runs 5] [--steps 6] [--configs image,c3] [--aovs depth,position,geo_normal,sh_normal]

image : the 96 x 64 range image of the README (bus, 128 range bins, 256 samples per pixel).  Neither layout fits the LDS window
        (6144 pixels), so both renders take global atomics by size.
c3    : C3 (car body, 1 x 1 film).  Both renders privatise their histogram in LDS; every path of the AOV render adds its K floats
        to the same K cells.
AOV renders do not roll, so every render is a stand-alone one on one handle, timed by the library (bf_stats: whole render,
wf_shade, wf_trace, tail).  Three modes per config, so that the cost of the flag can be told from what it brings along:
    lean      the plain render as bench.py runs it (the lean kernels where scene and launch fit their profile)
    general   the plain render on a handle created under BF_LEAN=0 (the general kernels: what the AOV variants are built from)
    aov       BF_FLAG_AOV
Prints one line per config and mode: medians over runs x steps of kernel_ms, shade_ms, trace_ms, tail_ms, the spread of
kernel_ms, kernel_ms relative to `general`, and the side rows' traffic per path (one store and one load of 4 bytes per stored
component: DESIGN.md 6i)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--configs", default="image,c3")
    ap.add_argument("--aovs", default="depth,position,geo_normal,sh_normal")
    args = ap.parse_args()
    import numpy as np
    import torch
    from beifong_amd import capi, scenes
    from beifong_amd.scenedesc import Transform4f as T
    import bench

    dev = torch.device("cuda", 0)
    lib = capi.load_library()
    AOV, STATS = capi.BF_FLAG_AOV, capi.BF_FLAG_STATS
    types = capi.aov_types(args.aovs.split(","))
    stored = sorted(set(int(t) for t in types if t < capi.BF_AOV_DUV_DX))
    row_bytes = 2 * 4 * sum(capi.AOV_TYPE_FLOATS[t] for t in stored)

    class A:       # the bench arguments Workload reads
        paths = tris = cpu_paths = streams = 0
        pulses = 64
        scaling = "weak"
        rolling = 0

    def image():
        sd, _ = scenes.bus_radar(n_tris=200_000, n_paths=1)
        pose = T.translate([0, 0, 0.3]) * T.rotate([1, 0, 0], 90) * T.rotate([0, 1, 0], 90)
        sd.set_perspective(pose, fov=60.0, near_clip=0.1, far_clip=100.0, film=(96, 64))
        sd.finalize()
        return sd, lambda i, flags: capi.make_launch(capi.BF_MODE_RANGE, 96 * 64 * 256, seed=1 + i, bins=128, bin_width=0.1, film=(96, 64),
                                                     spp=256, flags=flags)

    def c3():
        a = A()
        a.config = "c3"
        w = bench.Workload(a, 0, 1, capi, scenes)
        return w.sd, w.launch

    def run_config(name, sd, launch):
        lean = capi.Scene(sd, lib)
        lean.set_aovs(types)
        os.environ["BF_LEAN"] = "0"
        general = capi.Scene(sd, lib)          # the tunables are read when a scene is created
        del os.environ["BF_LEAN"]
        modes = {"lean": (lean, 0), "general": (general, 0), "aov": (lean, AOV)}
        hist = torch.zeros(lean.channels(launch(0, AOV)), dtype=torch.float32, device=dev)
        keys = ("kernel_ms", "shade_ms", "trace_ms", "tail_ms")
        ms = {m: {k: [] for k in keys} for m in modes}
        variant = {}

        def region(mode, keep):
            g, flags = modes[mode]
            for i in range(args.steps):
                hist.zero_()
                torch.cuda.synchronize()
                st = g.render_device(launch(i, flags | STATS), hist.data_ptr(), want_stats=True)
                variant[mode] = st.kernel_variant
                if keep:
                    for k in keys:
                        ms[mode][k].append(getattr(st, k))

        for m in modes:                          # warm-up (pools, launch plans, side rows)
            region(m, False)
        order = list(modes)
        for r in range(args.runs):
            for m in (order if r % 2 == 0 else order[::-1]):
                region(m, True)
        base = np.median(ms["general"]["kernel_ms"])
        lp = launch(0, AOV)
        print(f"{name}: {int(lp.n_paths)} paths, {lean.channels(launch(0, 0))} floats plain, {lean.channels(lp)} with the AOVs "
              f"({args.aovs}: K = {capi.aov_floats(types, lib)}, side rows {row_bytes} bytes per path)", flush=True)
        for m in modes:
            k = ms[m]["kernel_ms"]
            print(f"  {m:8s} variant {variant[m]:2d}  kernel {np.median(k):8.3f} ms ({min(k):.3f}..{max(k):.3f})  shade {np.median(ms[m]['shade_ms']):8.3f}"
                  f"  trace {np.median(ms[m]['trace_ms']):8.3f}  tail {np.median(ms[m]['tail_ms']):8.3f}  kernel / general {np.median(k) / base:.3f}", flush=True)
        lean.close()
        general.close()

    for cfg in args.configs.split(","):
        if cfg == "image":
            run_config(cfg, *image())
        elif cfg == "c3":
            run_config(cfg, *c3())
        else:
            raise SystemExit(f"unknown config {cfg}")


if __name__ == "__main__":
    main()
