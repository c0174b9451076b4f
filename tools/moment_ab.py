"""Developer A/B: renders with and without second moments (BF_FLAG_MOMENT) on the bench configs, interleaved run by run.

    python tools/moment_ab.py [--runs 5] [--steps 20] [--configs c2roll,c2sa,c2iso,c3iso,c4iso,c5]

c2roll : bench.py's C2 region: `steps` rolling renders over 2 handles (clones of one scene), flushed, per step
c2sa   : the same steps as stand-alone renders over 8 handles (every step its own tail)
c2iso / c3iso / c4iso : one stand-alone render at a time on one handle (C2, C3, a C4 shard), wall time per render
c5     : one C5 sweep (64 pulses of 2^20 paths, batched rolling launches over 4 handles), per sweep
Prints one line per config and mode: median and spread (min..max) over the runs, and moment / plain of the medians.
The histograms of a moment render are 5 + 2 (bins + 3) floats wide instead of 5 + bins (include/beifong_hip.h)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--configs", default="c2roll,c2sa,c2iso,c3iso,c4iso,c5")
    ap.add_argument("--mode", default="both", choices=["both", "plain", "moment"], help="one mode only: profiling runs (rocprofv3)")
    args = ap.parse_args()
    import numpy as np
    import torch
    from beifong_amd import capi, scenes
    import bench

    dev = torch.device("cuda", 0)
    lib = capi.load_library()
    MOMENT = capi.BF_FLAG_MOMENT

    class A:       # the bench arguments Workload reads
        paths = tris = cpu_paths = streams = 0
        pulses = 64
        scaling = "weak"

    def workload(cfg, rolling):
        a = A()
        a.config, a.rolling = cfg, rolling
        return bench.Workload(a, 0, 1, capi, scenes)


    def run_region(name, w, n_streams, rolling, steps, iso=False):
        first = capi.Scene(w.sd, lib)
        handles = [first] + [first.clone() for _ in range(n_streams - 1)]
        n_chan = first.channels(w.launch(0, MOMENT))          # the wider of the two layouts: both modes write into the same buffers
        hists = torch.zeros((max(steps, 2), n_chan * (w.n_pulses if w.sweep else 1)), dtype=torch.float32, device=dev)
        streams = [torch.cuda.Stream(dev) for _ in range(n_streams)]
        roll = capi.BF_FLAG_ROLLING if rolling else 0

        def region(flags):
            hists.zero_()
            for s in streams:
                s.wait_stream(torch.cuda.current_stream(dev))
            torch.cuda.synchronize()
            t = time.perf_counter()
            for i in range(steps):
                l = w.launch(i, flags | roll)
                if not w.sweep:
                    j = i % n_streams
                    with torch.cuda.stream(streams[j]):
                        handles[j].render_device(l, hists[i].data_ptr(), stream=streams[j].cuda_stream)
                else:
                    k = w.n_pulses // n_streams         # one batch of k pulses per handle, as bench.py deals them
                    for c in range(n_streams):
                        with torch.cuda.stream(streams[c]):
                            handles[c].render_batch_device(l, k, hists[i].data_ptr() + 4 * n_chan * k * c,
                                                           offsets=w.offsets[k * c:k * (c + 1)], stream=streams[c].cuda_stream)
                if iso:
                    torch.cuda.synchronize()
            for j in range(n_streams if rolling else 0):
                handles[j].flush(stream=streams[j].cuda_stream)
            torch.cuda.synchronize()
            return (time.perf_counter() - t) * 1e3 / steps

        modes = {"both": (0, MOMENT), "plain": (0,), "moment": (MOMENT,)}[args.mode]
        for flags in modes:          # warm-up (plans, pools)
            region(flags)
        ms = {0: [], MOMENT: []}
        for r in range(args.runs):
            for flags in (modes if r % 2 == 0 else modes[::-1]):
                ms[flags].append(region(flags))
        for h in handles:
            h.close()
        if len(modes) == 1:
            print(f"{name:8s} {args.mode} {np.median(ms[modes[0]]):8.3f} ms", flush=True)
            return
        e, f = np.median(ms[0]), np.median(ms[MOMENT])
        print(f"{name:8s} plain {e:8.3f} ms ({min(ms[0]):.3f}..{max(ms[0]):.3f})  moment {f:8.3f} ms ({min(ms[MOMENT]):.3f}..{max(ms[MOMENT]):.3f})"
              f"  moment/plain {f / e:.3f}", flush=True)

    for cfg in args.configs.split(","):
        if cfg == "c2roll":
            run_region(cfg, workload("c2", 1), 2, True, args.steps)
        elif cfg == "c2sa":
            run_region(cfg, workload("c2", 0), 8, False, args.steps)
        elif cfg == "c2iso":
            run_region(cfg, workload("c2", 0), 1, False, 5, iso=True)
        elif cfg == "c3iso":
            run_region(cfg, workload("c3", 0), 1, False, 10, iso=True)
        elif cfg == "c4iso":
            run_region(cfg, workload("c4shard", 0), 1, False, 10, iso=True)
        elif cfg == "c5":
            run_region(cfg, workload("c5", 1), 4, True, 2)
        else:
            raise SystemExit(f"unknown config {cfg}")


if __name__ == "__main__":
    main()
