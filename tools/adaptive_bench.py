#!/usr/bin/env python3
"""Adaptive sampling against the fixed sample count (rtu_render_frame_adaptive_device vs rtu_render_frame_device), one JSON line per
workload: milliseconds per frame of each (HIP events around whole frames on one stream, after warm-up frames, median of --frames),
mean samples per pixel of the adaptive frame, traced primary rays / (samples x pixels), and the cost of an adaptive frame whose
min_samples == samples (every pixel to the maximum) relative to the fixed frame.

Traced primary rays: a pixel that stops at n was traced ceil(n / B) * B times (at most `samples`) with batches of B samples — the exact
count of the counting variant (tests/test_gpu_adaptive.py, test_stopped_pixels_trace_nothing), here computed from the count image.

usage: tools/adaptive_bench.py [--frames 5] [--warmup 2] [--samples 64] [--out profiles/r04_adaptive.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (name, golden tag of the scene, resolution, gather bounces)
WORKLOADS = [("teapot1_s2 recipe S 1920x1080", "teapot1_s2_160x90", (1920, 1080), 0),
             ("p11_1080 recipe P (config 5)", "p11_1080", None, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    pkg = g.load_package()
    torch.cuda.set_device(0)
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream()
    lines = []
    for name, tag, size, gather in WORKLOADS:
        scene = pkg.Scene.from_blob_file(os.path.join(REPO, "tests", "golden", tag, "scene.rtus.gz"))
        if size is None:
            meta = json.load(open(os.path.join(REPO, "tests", "golden", tag, "meta.json")))
            size = (meta["width"], meta["height"])
        W, H = size
        ctx.upload(scene)
        fr = pkg.frame_setup(scene.desc.camera, W, H, samples=args.samples, gather_bounces=gather)
        pixels = W * H
        rgbz = torch.empty(pixels * 4, dtype=torch.float32, device="cuda")
        counts = torch.empty(pixels, dtype=torch.uint8, device="cuda")
        ad = pkg.adaptive_defaults()
        full = pkg.adaptive_defaults(min_samples=args.samples)

        def timed(render):
            for _ in range(args.warmup):
                render()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.frames):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                render()
                e1.record(stream)
                e1.synchronize()
                if pkg.hip.rtu_frame_status(ctx._h) != pkg.RTU_OK:
                    raise SystemExit("%s: a frame did not complete" % name)
                ms.append(e0.elapsed_time(e1))
            return statistics.median(ms), ms

        def fixed():
            ctx.render_device(fr, rgbz.data_ptr(), stream.cuda_stream)

        def adaptive(desc):
            return lambda: ctx._check(pkg.hip.rtu_render_frame_adaptive_device(ctx._h, pkg.ctypes.byref(fr), pkg.ctypes.byref(desc), rgbz.data_ptr(),
                                                                              counts.data_ptr(), stream.cuda_stream))

        fixed_ms, fixed_all = timed(fixed)
        ad_ms, ad_all = timed(adaptive(ad))
        n = counts.cpu().numpy().astype(np.int64)
        full_ms, full_all = timed(adaptive(full))
        batch = max(1, min(pkg.RTU_MAX_BATCH, (1 << 25) // pixels, args.samples))
        traced = int(np.minimum(args.samples, batch * ((n + batch - 1) // batch)).sum())
        line = {"workload": name, "tag": tag, "width": W, "height": H, "max_samples": args.samples, "gather_bounces": gather,
                "min_samples": ad.min_samples, "increment": ad.increment, "target_variance": round(float(ad.target_variance), 6), "batch": batch,
                "fixed_ms": round(fixed_ms, 3), "adaptive_ms": round(ad_ms, 3), "speedup": round(fixed_ms / ad_ms, 3),
                "mean_spp": round(float(n.mean()), 3), "pixels_at_min": round(float((n == ad.min_samples).mean()), 4),
                "pixels_at_max": round(float((n == args.samples).mean()), 4),
                "traced_primary_ratio": round(traced / (args.samples * pixels), 4),
                "all_max_ms": round(full_ms, 3), "all_max_over_fixed": round(full_ms / fixed_ms, 4),
                "runs_ms": {"fixed": [round(x, 3) for x in fixed_all], "adaptive": [round(x, 3) for x in ad_all], "all_max": [round(x, 3) for x in full_all]}}
        print(json.dumps(line), flush=True)
        lines.append(line)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
