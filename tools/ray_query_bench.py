#!/usr/bin/env python3
"""Rays per second of the ray queries (rtu_trace_rays_device / rtu_occluded_rays_device), one JSON line: the 1920x1080 camera rays of
teapot2_1080 and p4_1080 in three orders — image order, 8x8-tile order (the order of the render's wavefronts), shuffled — for both
entry points and both walks. Each figure is the median over `reps` launches, every launch bracketed by HIP events on one stream,
after `warmup` launches that are not counted. For comparison the primary phase of a recipe-W frame of the same camera on the same
build: the launches of k_primary, k_primary2c and k_primary2, bracketed by rtu_probe_kernel (that phase also shades its hits).

--sorted: instead, what sorting a shuffled batch on the GPU buys (tools/sorted_legs.py): per scene and entry point (fast walk) the
shuffled camera rays (a) as they are, (b) rtu_ray_order_device + gather + the query + scatter as one region, (c) those parts one by
one, and the image-order batch beside them; every timed sorted launch is compared byte for byte with the unsorted answers.
--scale k fires the camera at k times the resolution (k * k times the rays): where the sort breaks even depends on the batch size.

usage: tools/ray_query_bench.py [--sorted [--scale 1]] [--reps 20] [--warmup 3] [--out profiles/r08_ray_queries.json]"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))

TAGS = ["teapot2_1080", "p4_1080"]


def orders(np, w, h):
    idx = np.arange(w * h, dtype=np.int64).reshape(h, w)
    hp, wp = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    pad = np.full((hp, wp), -1, np.int64)
    pad[:h, :w] = idx
    tiles = pad.reshape(hp // 8, 8, wp // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    return {"image": idx.reshape(-1), "tiles8x8": tiles[tiles >= 0], "shuffled": np.random.RandomState(1).permutation(w * h)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--sorted", action="store_true", help="time a shuffled batch as it is against order + gather + query + scatter")
    ap.add_argument("--scale", type=int, default=1, help="with --sorted: the camera at this multiple of the fixture's resolution")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    pkg = g.load_package()
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    out = {"tool": "ray_query_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scenes": []}
    if args.sorted:
        from sorted_legs import sorted_legs
        out["mode"] = "sorted"
        for tag in TAGS:
            gd = Golden(tag)
            scene = gd.scene(pkg)
            W, H = gd.width * args.scale, gd.height * args.scale
            ctx.upload(scene)
            rays = pkg.camera_rays(pkg.frame_setup(scene.desc.camera, W, H))
            n = rays.size
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda:0")
            d_image, d_shuffled = dev(rays), dev(rays[np.random.RandomState(1).permutation(n)])
            row = {"scene": tag, "width": W, "height": H, "queries": {}}
            for entry, nbytes in (("closest", 48), ("occluded", 1)):
                query = ctx.trace_rays_device if entry == "closest" else ctx.occluded_device
                row["queries"][entry] = sorted_legs(pkg, ctx, torch, stream, n, d_image, d_shuffled, None, None, nbytes,
                                                    lambda r, k, o: query(r, n, o, stream.cuda_stream), args.reps, args.warmup, False)
            out["scenes"].append(row)
        line = json.dumps(out)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")
        ctx.close()
        return
    for tag in TAGS:
        gd = Golden(tag)
        scene = gd.scene(pkg)
        W, H = gd.width, gd.height
        ctx.upload(scene)
        frame = pkg.frame_setup(scene.desc.camera, W, H)
        rays = pkg.camera_rays(frame)
        n = rays.size
        d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
        d_occ = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        row = {"scene": tag, "width": W, "height": H, "rays": int(n), "queries": {}}
        for oname, order in orders(np, W, H).items():
            d_rays = torch.from_numpy(np.ascontiguousarray(rays[order]).view(np.uint8).copy()).to("cuda:0")
            for entry in ("closest", "occluded"):
                for ref in (False, True):
                    def launch():
                        if entry == "closest":
                            ctx.trace_rays_device(d_rays.data_ptr(), n, d_hits.data_ptr(), stream.cuda_stream, reference_walk=ref)
                        else:
                            ctx.occluded_device(d_rays.data_ptr(), n, d_occ.data_ptr(), stream.cuda_stream, reference_walk=ref)
                    for _ in range(args.warmup):
                        launch()
                    stream.synchronize()
                    ms = []
                    for _ in range(args.reps):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record(stream)
                        launch()
                        e1.record(stream)
                        e1.synchronize()
                        ms.append(e0.elapsed_time(e1))
                    med = statistics.median(ms)
                    row["queries"]["%s/%s/%s" % (oname, entry, "reference" if ref else "fast")] = {
                        "median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "mrays_per_s": n / med / 1e3}
            del d_rays
        # the primary phase of a render of the same camera
        d_img = pkg.hip.rtu_device_alloc(ctx._h, n * 16)
        for _ in range(args.warmup):
            ctx.render_device(frame, d_img)
            ctx.frame_status()
        phase = {}
        for slot in ("k_primary", "k_primary2c", "k_primary2"):
            ctx.probe_kernel(slot)
            for _ in range(args.reps):
                ctx.render_device(frame, d_img)
                ctx.frame_status()
            ms, launches = ctx.probe_read()
            phase[slot] = {"ms_per_frame": ms / args.reps, "launches_per_frame": launches / args.reps}
        ctx.probe_kernel(None)
        pkg.hip.rtu_device_free(ctx._h, d_img)
        total = sum(v["ms_per_frame"] for v in phase.values())
        row["render_primary_phase"] = dict(phase, total_ms=total, mrays_per_s=n / total / 1e3 if total > 0 else None)
        out["scenes"].append(row)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
