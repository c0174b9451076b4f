"""Cost of the converge call's own work: rounds of R moment renders through Scene.render_converge_device (accumulate + statistic
+ one event wait per round) against the same batches issued by hand (Scene.render_batch_device, no check), interleaved, wall clock
around a synchronised region; then the statistic entry alone (allocation, three kernels, wait) on two layouts.

    python tools/converge_ab.py [--shape c2|c5] [--paths N] [--rounds 4] [--renders 4] [--reps 5] [--arm both|by_hand]

--arm by_hand uses nothing a tree without the converge entries lacks, so the same file runs from a checkout of the parent commit
(python path/to/this/converge_ab.py --root <that checkout> --arm by_hand) for the by-hand figure of the parent's library.
"""
import argparse
import json
import os
import sys
import time

import numpy as np



def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose beifong_amd is measured")
    ap.add_argument("--shape", default="c2", choices=["c2", "c5"], help="bench.py's C2 (range, 256 bins) or C5 (receive I/Q, 1024 fast-time bins) scene")
    ap.add_argument("--arm", default="both", choices=["both", "by_hand"])
    ap.add_argument("--paths", type=int, default=0, help="per render; 0 = 2^22 (c2), 2^20 (c5)")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--renders", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.root))
    from beifong_amd import capi, scenes
    if a.shape == "c2":
        a.paths = a.paths or 1 << 22
        sd, lp = scenes.bus_radar(n_paths=a.paths)      # the C2 scene and launch, at --paths per render
    else:
        a.paths = a.paths or 1 << 20
        lam0 = 8.6e6                                    # (bench.py --config c5)
        sd, lp = scenes.bus_receive(n_tris=200_000, n_paths=a.paths, t_bins=1024, dr=0.03, seed=4, lambda_band_nm=(lam0 * 0.999, lam0 * 1.001))
        lp.mode = capi.BF_MODE_RECEIVE_IQ
    lp.flags |= capi.BF_FLAG_MOMENT
    g = capi.Scene(sd)
    n = g.channels(lp)
    acc = torch.zeros(n, dtype=torch.float32, device="cuda")
    blocks = torch.zeros((a.renders, n), dtype=torch.float32, device="cuda")

    def converge():
        return g.render_converge_device(lp, acc.data_ptr(), 0.0, floor=0.01, round_renders=a.renders, max_rounds=a.rounds)

    def by_hand():
        for r in range(a.rounds):
            blocks.zero_()
            # (the converge call's seeds: capi.converge_seeds)
            g.render_batch_device(lp, a.renders, blocks.data_ptr(), seeds=[lp.seed + (r * a.renders + j) * a.paths for j in range(a.renders)])

    arms = (("converge", converge), ("by_hand", by_hand)) if a.arm == "both" else (("by_hand", by_hand),)
    t = {name: [] for name, _ in arms}
    for rep in range(a.reps + 1):
        for name, fn in arms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:                                     # the first repetition warms up
                t[name].append((time.perf_counter() - t0) * 1e3 / a.rounds)
    out = {"shape": a.shape, "root": os.path.relpath(a.root), "paths_per_render": a.paths, "renders_per_round": a.renders, "rounds": a.rounds, "channels": n,
           "ms_per_round": {k: {"median": float(np.median(v)), "min": min(v), "max": max(v)} for k, v in t.items()}}
    # the statistic entry alone (hipMalloc + hipHostMalloc + three kernels + wait): an upper bound of the kernels' time
    rng = np.random.default_rng(1)
    for name, lm in () if a.arm != "both" else ((a.shape + " layout", lp),
                     ("film 96 x 64 x 128 bins", capi.make_launch(capi.BF_MODE_RANGE, 96 * 64 * 4, bins=128, bin_width=1.0, flags=capi.BF_FLAG_MOMENT,
                                                                  film=(96, 64), spp=4))):
        h = torch.from_numpy(rng.uniform(1.0, 2.0, g.channels(lm)).astype(np.float32)).cuda()
        ms = []
        for rep in range(6):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            g.converge_statistic_device(lm, h.data_ptr(), 0.01)
            ms.append((time.perf_counter() - t0) * 1e3)
        out.setdefault("statistic_entry_ms", {})[name] = {"floats": int(h.numel()), "median": float(np.median(ms[1:])), "min": min(ms[1:])}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
