#!/usr/bin/env python3
"""Time of an adaptive sensor render (rtu_render_sensor_adaptive_device) against the fixed one (rtu_render_sensor_device), one JSON
line: the 2048x1024 equirectangular sensor of tools/sensor_bench.py on Project10/scene.xml (recipe S) and Project11/scene.xml (recipe P)
at 64 samples with the reference's constants (min_samples 8, increment 1, target 0.005).

  fixed / adaptive   host clock around each call, which returns when the image is complete; the two ALTERNATE in one run (fixed,
                     adaptive, fixed, ...), median, min and max of `reps` each after `warmup` rounds.
  overhead           min_samples == samples (every pixel takes every sample: the fixed render's bytes, checked) against the fixed render,
                     alternating in the same way: what the new layer costs where it saves nothing.
  mean_samples       the mean of the count image; traced_fraction: the rays the batches traced (rtu_debug_sensor_adaptive_trace:
                     the sum of live pixels x samples) over samples x pixels.

usage: tools/sensor_adaptive_bench.py [--reps 5] [--warmup 2] [--samples 64] [--width 2048] [--height 1024] [--out FILE]
(profiles/r25_sensor_adaptive.json)"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

# (golden holding the scene, its name, gather_bounces)
WORKLOADS = [("p10_s4_160x120", "Project10/scene.xml", 0), ("p11_p2_120x68", "Project11/scene.xml", 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    from test_sensor_host import camera_basis
    pkg = g.load_package()
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    W, H, S = args.width, args.height, args.samples
    pixels = W * H
    out = {"tool": "sensor_adaptive_bench", "width": W, "height": H, "samples": S, "reps": args.reps, "warmup": args.warmup,
           "device": pkg.device_info(0)["name"], "workloads": []}

    def spread(ms):
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    for tag, name, gather in WORKLOADS:
        scene = Golden(tag).scene(pkg)
        ctx.upload(scene)
        pos, right, up, fwd = camera_basis(scene)
        d = pkg.sensor_desc("equirect", W, H, pos, right, up, fwd, samples=S, gather_bounces=gather)
        ad = pkg.adaptive_defaults()  # the reference's 8 / 1 / 0.005
        full = pkg.adaptive_defaults(min_samples=S)
        d_fixed = torch.zeros(pixels * 4, dtype=torch.float32, device="cuda:0")
        d_img = torch.zeros(pixels * 4, dtype=torch.float32, device="cuda:0")
        d_counts = torch.zeros(pixels, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

        def fixed():
            t0 = time.perf_counter()
            ctx.render_sensor_device(d, d_fixed.data_ptr(), stream.cuda_stream)
            return (time.perf_counter() - t0) * 1e3

        def adaptive(a):
            t0 = time.perf_counter()
            ctx.render_sensor_adaptive_device(d, d_img.data_ptr(), d_counts.data_ptr(), a, stream.cuda_stream)
            return (time.perf_counter() - t0) * 1e3

        def alternate(a):
            for _ in range(args.warmup):
                fixed()
                adaptive(a)
            f, v = [], []
            for _ in range(args.reps):
                f.append(fixed())
                v.append(adaptive(a))
            return spread(f), spread(v)
        row = {"scene": name, "recipe": "P" if gather else "S", "min_samples": ad.min_samples, "increment": ad.increment,
               "target_variance": float(ad.target_variance)}
        row["fixed"], row["adaptive"] = alternate(ad)
        trace = ctx.sensor_adaptive_trace()
        counts = d_counts.cpu().numpy()
        row["fixed_over_adaptive"] = row["fixed"]["median_ms"] / row["adaptive"]["median_ms"]
        row["mean_samples"] = float(counts.mean())
        row["pixels_at_min_samples"] = float((counts == ad.min_samples).mean())
        row["batches"] = trace
        row["traced_fraction"] = sum(l * b for l, b in trace) / float(S * pixels)
        f, v = alternate(full)
        row["overhead"] = {"fixed": f, "adaptive_min_eq_samples": v, "adaptive_over_fixed": v["median_ms"] / f["median_ms"],
                           "equals_fixed": bool(np.array_equal(d_img.cpu().numpy().view(np.uint32), d_fixed.cpu().numpy().view(np.uint32))),
                           "batches": ctx.sensor_adaptive_trace()}
        out["workloads"].append(row)
        del d_fixed, d_img, d_counts
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
