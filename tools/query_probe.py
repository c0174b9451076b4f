#!/usr/bin/env python3
"""Rates of the device-side queries on the C2 scene (developer tool; DESIGN.md "Device-side plugin queries").

For 2^20 and 2^24 queries: ray_intersect_device / trace_any_device on device buffers against the host forms (which stage
the rays and copy the results back), and the BSDF eval + pdf, BSDF sample and emitter sample_direction probes (device
forms).  Device forms are timed with HIP events around the call on one stream after a warm-up; host forms with the wall
clock around the synchronous call.  A and B alternate within one process, `--reps` rounds each; the median is printed as
one JSON line per measurement.
usage: query_probe.py [--reps 5] [--log2 20 24]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--log2", type=int, nargs="+", default=[20, 24])
    args = ap.parse_args()
    import torch
    from beifong_amd import capi, scenes
    sd, _ = scenes.bus_radar(n_tris=200_000, n_paths=1 << 20, bins=256, dr=0.1, seed=1)
    g = capi.Scene(sd)
    stream = torch.cuda.Stream()
    s = stream.cuda_stream
    for lg in args.log2:
        n = 1 << lg
        rng = np.random.default_rng(lg)
        rays = np.zeros((n, 8), np.float32)
        tgt = rng.uniform([5, -4, 0], [20, 4, 4], (n, 3))
        o = np.tile(np.array([0.0, 0.0, 0.3]), (n, 1))
        d = tgt - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        rays[:, 0:3], rays[:, 3], rays[:, 4:7], rays[:, 7] = o, 1e-4, d, np.inf
        wi = rng.normal(size=(n, 3))
        wi /= np.linalg.norm(wi, axis=1, keepdims=True)
        bsdf_rows = np.concatenate([wi, rng.random((n, 3))], 1).astype(np.float32)
        em_rows = np.concatenate([rng.uniform(-5, 5, (n, 3)), rng.random((n, 2))], 1).astype(np.float32)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        t_rays, t_b, t_e = dev(rays), dev(bsdf_rows), dev(em_rows)
        t_mat = torch.zeros(n, dtype=torch.int32, device="cuda")
        si = torch.empty((n, capi.BF_SI_FLOATS), dtype=torch.float32, device="cuda")
        hit = torch.empty(n, dtype=torch.uint8, device="cuda")
        out = torch.empty((n, 8), dtype=torch.float32, device="cuda")
        mats = np.zeros(n, np.uint32)
        device_forms = {
            "ray_intersect_device": lambda: g.ray_intersect_device(n, t_rays.data_ptr(), si.data_ptr(), stream=s),
            "trace_any_device": lambda: g.trace_any_device(n, t_rays.data_ptr(), hit.data_ptr(), stream=s),
            "bsdf_eval_pdf_device": lambda: g.bsdf_eval_pdf_device(n, t_mat.data_ptr(), t_b.data_ptr(), out.data_ptr(), stream=s),
            "bsdf_sample_device": lambda: g.bsdf_sample_device(n, t_mat.data_ptr(), t_b.data_ptr(), out.data_ptr(), stream=s),
            "emitter_sample_direction_device": lambda: g.emitter_sample_direction_device(0, n, t_e.data_ptr(), out.data_ptr(), stream=s),
        }
        host_forms = {
            "ray_intersect": lambda: g.ray_intersect(rays),
            "trace_any": lambda: g.trace_any(rays),
        }
        times = {k: [] for k in list(device_forms) + list(host_forms)}
        for f in list(device_forms.values()) + list(host_forms.values()):      # warm-up
            f()
        torch.cuda.synchronize()
        for _ in range(args.reps):
            for name in ("ray_intersect", "trace_any"):          # A (device form) and B (host form) alternate
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                device_forms[name + "_device"]()
                b.record(stream)
                b.synchronize()
                times[name + "_device"].append(a.elapsed_time(b))
                t0 = time.perf_counter()
                host_forms[name]()
                times[name].append((time.perf_counter() - t0) * 1e3)
            for name in ("bsdf_eval_pdf_device", "bsdf_sample_device", "emitter_sample_direction_device"):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(stream)
                device_forms[name]()
                b.record(stream)
                b.synchronize()
                times[name].append(a.elapsed_time(b))
        for name, ts in times.items():
            ms = statistics.median(ts)
            print(json.dumps(dict(query=name, n=n, ms_median=round(ms, 4), ms_min=round(min(ts), 4), reps=len(ts),
                                  mqueries_per_s=round(n / ms / 1e3, 1), clock="hip events" if name.endswith("_device") else "wall")))
        del mats


if __name__ == "__main__":
    main()
