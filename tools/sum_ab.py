"""Developer A/B: renders with and without exact sums (BF_FLAG_EXACT_SUM) on the full-size bench scenes, interleaved run by run,
with the per-kernel times of BF_FLAG_STATS.

    python tools/sum_ab.py [--runs 5] [--steps 6] [--configs c4,c2]

c4 : one C4 shard (bus + car + motorbike, 4096 range bins, 2^19 paths) per render.  4101 cells of 72 bytes do not fit the LDS:
     the exact-sum render takes GLOBAL limbs by size (its five base channels through the workgroup's table), the plain one
     privatises its histogram in LDS.
c2 : C2 (bus, 256 range bins).  261 cells: the limbs are privatised in LDS.
Exact sums do not roll, so every render is a stand-alone one on one handle (bench.py's "iso" probe), timed by the library
(bf_stats: whole render — the limbs' memset and the resolve kernel included — wf_shade, wf_trace, tail).  Four modes per config, so
that the cost of the flag can be told from what it brings along:
    lean        the plain render as bench.py runs it (lean kernels, base channels in registers)
    general     the plain render on a handle created under BF_LEAN=0 (the general kernels: what the exact-sum variants are built from)
    general_ga  ... with BF_FLAG_GLOBAL_ATOMICS (fp32 atomics in global memory)
    exact_sum   BF_FLAG_EXACT_SUM
Prints one line per config and mode: medians over runs x steps of kernel_ms, shade_ms, trace_ms, tail_ms, the spread of kernel_ms
and kernel_ms relative to `lean`."""
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
    args = ap.parse_args()
    import numpy as np
    import torch
    from beifong_amd import capi, scenes
    import bench

    dev = torch.device("cuda", 0)
    lib = capi.load_library()
    SUM, GA, STATS = capi.BF_FLAG_EXACT_SUM, capi.BF_FLAG_GLOBAL_ATOMICS, capi.BF_FLAG_STATS

    class A:       # the bench arguments Workload reads
        paths = tris = cpu_paths = streams = 0
        pulses = 64
        scaling = "weak"
        rolling = 0

    def run_config(name, cfg):
        a = A()
        a.config = cfg
        w = bench.Workload(a, 0, 1, capi, scenes)
        lean = capi.Scene(w.sd, lib)
        os.environ["BF_LEAN"] = "0"
        general = capi.Scene(w.sd, lib)          # the tunables are read when a scene is created
        del os.environ["BF_LEAN"]
        modes = {"lean": (lean, 0), "general": (general, 0), "general_ga": (general, GA), "exact_sum": (lean, SUM)}
        hist = torch.zeros(lean.channels(w.launch(0, SUM)), dtype=torch.float32, device=dev)
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
        base = np.median(ms["lean"]["kernel_ms"])
        lp = w.launch(0, SUM)
        print(f"{name}: {int(lp.n_paths)} paths, {lean.channels(lp)} cells", flush=True)
        for m in modes:
            k = ms[m]["kernel_ms"]
            print(f"  {m:11s} variant {variant[m]:2d}  kernel {np.median(k):8.3f} ms ({min(k):.3f}..{max(k):.3f})  shade {np.median(ms[m]['shade_ms']):8.3f}"
                  f"  trace {np.median(ms[m]['trace_ms']):8.3f}  tail {np.median(ms[m]['tail_ms']):8.3f}  kernel / lean {np.median(k) / base:.3f}", flush=True)
        lean.close()
        general.close()

    for cfg in args.configs.split(","):
        if cfg == "c4":
            run_config(cfg, "c4shard")
        elif cfg == "c2":
            run_config(cfg, "c2")
        else:
            raise SystemExit(f"unknown config {cfg}")


if __name__ == "__main__":
    main()
