#!/usr/bin/env python3
"""What the surface records cost (rtu_frame_surface_device, rtu_ray_surface_device), one JSON line: a frame at 1920x1080, the guides
with the record against the guides without it. Every figure is the median over `reps` regions bracketed by HIP events on one stream,
after `warmup` regions that are not counted; the two entries of a pair ALTERNATE region by region in the same run.

  frame   rtu_frame_surface_device against rtu_frame_features_device (rays generated in the kernel)
  rays    rtu_ray_surface_device against rtu_ray_features_device on the uploaded rtu_camera_rays of the same frame
  floor   a device copy of the 32 bytes per pixel the record adds
The hits and albedo of both entries are compared byte for byte, and the record's share of triangle-mesh hits is reported.

usage: tools/surface_bench.py [--reps 20] [--warmup 3] [--tags p11_1080,teapot2_1080] [--out profiles/r26_surface.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tags", default="p11_1080,teapot2_1080")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("surface_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    out = {"tool": "surface_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scenes": {}}

    def alternating(launches):
        """launches: name -> callable; the regions of all of them in turn, `reps` times."""
        for _ in range(args.warmup):
            for f in launches.values():
                f()
        stream.synchronize()
        ms = {k: [] for k in launches}
        for _ in range(args.reps):
            for k, f in launches.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
        return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)} for k, v in ms.items()}

    for tag in args.tags.split(","):
        gd = Golden(tag)
        scene = gd.scene(pkg)
        W, H = gd.width, gd.height
        n = W * H
        ctx.upload(scene)
        frame = pkg.frame_setup(scene.desc.camera, W, H)
        rays = pkg.camera_rays(frame)
        d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to("cuda:0")
        d_hits = [torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0") for _ in range(4)]
        d_alb = [torch.zeros((n, 4), dtype=torch.float32, device="cuda:0") for _ in range(4)]
        d_surf = [torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        s = stream.cuda_stream
        with torch.cuda.stream(stream):
            r = alternating({
                "frame_features_device": lambda: ctx.frame_features_device(frame, d_hits[0].data_ptr(), d_alb[0].data_ptr(), s),
                "frame_surface_device": lambda: ctx.frame_surface_device(frame, d_hits[1].data_ptr(), d_alb[1].data_ptr(), d_surf[0].data_ptr(), s),
                "ray_features_device": lambda: ctx.ray_features_device(d_rays.data_ptr(), n, d_hits[2].data_ptr(), d_alb[2].data_ptr(), s),
                "ray_surface_device": lambda: ctx.ray_surface_device(d_rays.data_ptr(), n, d_hits[3].data_ptr(), d_alb[3].data_ptr(),
                                                                     d_surf[1].data_ptr(), s),
                "copy_32B_per_pixel": lambda: d_surf[2].copy_(d_surf[0], non_blocking=True),
            })
        stream.synchronize()
        r["hits_equal"] = bool(torch.equal(d_hits[0], d_hits[1]) and torch.equal(d_hits[0], d_hits[2]) and torch.equal(d_hits[0], d_hits[3]))
        r["albedo_equal"] = bool(torch.equal(d_alb[0].view(torch.int32), d_alb[1].view(torch.int32)) and
                                 torch.equal(d_alb[0].view(torch.int32), d_alb[3].view(torch.int32)))
        r["surface_equal"] = bool(torch.equal(d_surf[0], d_surf[1]))
        surf = d_surf[0].cpu().numpy().view(pkg.surface_dtype())
        r["mesh_hit_share"] = float((surf["mesh"] >= 0).mean())
        r["frame_surface_over_features"] = r["frame_surface_device"]["median_ms"] / r["frame_features_device"]["median_ms"]
        r["ray_surface_over_features"] = r["ray_surface_device"]["median_ms"] / r["ray_features_device"]["median_ms"]
        r["width"], r["height"] = W, H
        out["scenes"][tag] = r
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(REPO, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
