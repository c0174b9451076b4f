"""Motion batches against the per-pulse motion sweep on a C5-shaped sweep: C2's bus geometry plus a second mesh
target (a car), gen-3 receive in BF_MODE_RECEIVE_IQ with a 1024-bin fast-time ADC, 64 pulses x 2^20 paths.  The bus approaches
at 5 m/s, the car drives away at 12 m/s while it turns; every pulse has its own pair of rigid transforms.

    python tools/motion_batch_ab.py [--reps 5] [--paths 1048576] [--streams 2]

Variants, interleaved rep by rep (handles built once, outside the timing; medians over the reps):
  per_pulse  one bf_scene_transform_meshes + one render per pulse, pulses rotating over the streams (render_motion_sweep
             per_pulse=True)
  batched    one motion batch per stream (bf_render_motion_batch_device: a geometry version per pulse; render_motion_sweep's
             default)
  offsets    the floor: the offset-batched sweep of a pure translation of both meshes (sweep.PulseSweeper, bf_batch.mesh_offsets)
Then wf_trace per render from a stats batch of one stream's share of the pulses, motion batch against offset batch: with up to 16
renders of 2^20 paths in a 2^24-path pool, up to 16 trees are live at once and may cost wf_trace cache hits."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import beifong_amd

beifong_amd.configure_runtime()
from beifong_amd import capi, meshgen, motion, scenes, sweep


def build(n_paths):
    lam0 = 8.6e6        # nm; the narrow band of tools/c5_sweep.py
    sd, lp = scenes.bus_receive(n_tris=200_000, n_paths=n_paths, t_bins=1024, dr=0.03, seed=4, lambda_band_nm=(lam0 * 0.999, lam0 * 1.001))
    lp.mode = capi.BF_MODE_RECEIVE_IQ
    mat = sd.add_roughconductor(alpha=0.1, twosided=True, specular_reflectance=1.0)
    v, f, _ = meshgen.car_body(60000, seed=2, with_normals=False)
    sd.add_mesh(meshgen.place(v, 15.0, (9.0, -3.0, 0.75)), f, mat)
    sd.finalize()
    return sd, lp


def poses(sd, n_pulses, pri=1e-3):
    meshes = [k for k, s in enumerate(sd.shapes) if s.type == capi.BF_SHAPE_MESH]
    bus, car = meshes[0], meshes[-1]
    s = sd.shapes[car]
    p = np.ctypeslib.as_array(s.positions, shape=(s.n_vertices, 3)).astype(np.float64)
    centre = 0.5 * (p.min(0) + p.max(0))
    xf = np.tile(motion.rigid()[None, None], (n_pulses, len(sd.shapes), 1, 1)).astype(np.float32)
    offsets = np.zeros((n_pulses, 3), np.float32)
    for i in range(n_pulses):
        t = i * pri
        xf[i, bus] = motion.rigid(t=(-5.0 * t, 0.0, 0.0))
        xf[i, car] = motion.about(motion.rotation([0, 0, 1], 20.0 * t), centre, (12.0 * t, 0.0, 0.0))      # 20 deg/s yaw
        offsets[i] = (-5.0 * t, 0.0, 0.0)
    return xf, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--paths", type=int, default=1 << 20)
    ap.add_argument("--pulses", type=int, default=64)
    ap.add_argument("--streams", type=int, default=2)
    a = ap.parse_args()
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    sd, lp = build(a.paths)
    n = a.pulses
    xf, offsets = poses(sd, n)
    S = max(1, min(a.streams, n))
    streams = [torch.cuda.Stream(dev) for _ in range(S)]
    first = capi.Scene(sd)
    handles = [first] + [first.clone() for _ in range(S - 1)]
    print(f"scene: {first.info().n_triangles} triangles, {len(sd.shapes)} shapes; {n} pulses x {a.paths} paths, {S} streams", flush=True)
    cube = torch.zeros((n, first.channels(lp)), dtype=torch.float32, device=dev)
    bounds = np.linspace(0, n, S + 1).astype(int)

    def per_pulse():
        cube.zero_()
        for s in streams:
            s.wait_stream(torch.cuda.current_stream(dev))
        for k in range(n):
            j = k % S
            with torch.cuda.stream(streams[j]):
                handles[j].transform_meshes(xf[k], stream=streams[j].cuda_stream)
                handles[j].render_device(lp, cube[k].data_ptr(), stream=streams[j].cuda_stream)
        for s in streams:
            s.synchronize()
        return cube.cpu().numpy()

    def batched():
        cube.zero_()
        for s in streams:
            s.wait_stream(torch.cuda.current_stream(dev))
        for j in range(S):
            lo, hi = int(bounds[j]), int(bounds[j + 1])
            with torch.cuda.stream(streams[j]):
                handles[j].render_motion_batch_device(lp, xf[lo:hi], cube[lo].data_ptr(), stream=streams[j].cuda_stream)
        for s in streams:
            s.synchronize()
        return cube.cpu().numpy()

    sw = sweep.PulseSweeper(sd, lp, S)

    def floor():
        return sw.render(offsets)

    variants = {"per_pulse": per_pulse, "batched": batched, "offsets": floor}
    for f in variants.values():          # warm-up: pools, launch plans, the motion arena
        f()
    times = {k: [] for k in variants}
    for rep in range(a.reps):
        for k, f in variants.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            times[k].append((time.perf_counter() - t) * 1e3)
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:9s}: median {med[k]:7.2f} ms over {len(v)} reps ({med[k] / n:.3f} ms per pulse); reps " + " ".join(f"{x:.2f}" for x in v), flush=True)
    print(f"batched / per_pulse = {med['batched'] / med['per_pulse']:.3f} (speed-up {med['per_pulse'] / med['batched']:.2f}x); "
          f"batched / offsets floor = {med['batched'] / med['offsets']:.3f}", flush=True)
    cb, cp = batched(), per_pulse()
    scale = float(np.abs(cp).max())
    print(f"max |batched - per_pulse| / max |cube| = {np.abs(cb - cp).max() / scale:.2e}; W equal: {np.array_equal(cb[:, 2::3], cp[:, 2::3])}", flush=True)
    sw.close()

    # wf_trace per render, one stream's share of the pulses in one stats batch each way
    m = int(bounds[1])
    h = torch.zeros((m, first.channels(lp)), dtype=torch.float32, device=dev)
    tr = {"motion": [], "offsets": []}
    for rep in range(a.reps):
        h.zero_()
        st = first.render_motion_batch_device(lp, xf[:m], h.data_ptr(), want_stats=True)
        tr["motion"].append(st.trace_ms / m)
        h.zero_()
        st2 = first.render_batch_device(lp, m, h.data_ptr(), offsets=offsets[:m], want_stats=True)
        tr["offsets"].append(st2.trace_ms / m)
    tm, to = float(np.median(tr["motion"])), float(np.median(tr["offsets"]))
    print(f"wf_trace per render ({m} renders per batch, stats runs): motion batch {tm:.3f} ms, offset batch {to:.3f} ms, "
          f"ratio {tm / to:.3f}; rays traced per render {st.n_rays_traced / m:.0f} vs {st2.n_rays_traced / m:.0f}", flush=True)
    for hd in reversed(handles):
        hd.close()


if __name__ == "__main__":
    main()
