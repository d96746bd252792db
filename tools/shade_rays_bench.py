#!/usr/bin/env python3
"""Time of a ray batch (rtu_shade_rays_device) against the render of the same camera, one JSON line: the 1920x1080 camera rays of
teapot2_1080 and p4_1080, in image order and shuffled, shaded with eye = the camera; and rtu_render_frame_device of that camera as a
single frame, in the same run. Each figure is the median over `reps` launches, every launch bracketed by HIP events on one stream,
after `warmup` launches that are not counted (they also settle the frame capacities and launch hints: rtu_frame_status after each).
Every timed launch of a ray batch is checked complete and writes to a buffer of its own; after the last one each buffer is compared
with the render (equals_render), so that nothing stands between the timed launches that is not there in the render's loop.
The ray form has no tile occupancy, no screen rectangles and no two-stage walk: on the teapot, where most of the image is background,
it is expected to be slower than the render. p4, where every ray has work and the recursion is real, is the honest comparison.

--sampled: the same for recipe S (rtu_shade_rays_sampled_device): the camera-sample rays and keys (rtu_camera_sample_rays, sample 0 of a
one-sample frame) of Project10/scene.xml and Project11/scene_glossy_soft.xml at 1920x1080 against rtu_render_frame_device of that frame
with samples = 1 — one sample image, the accumulation and the resolve.

--paths: the same for recipe P (rtu_shade_rays_paths_device): the camera-sample rays and keys of Project11/scene.xml and
Project10/scene.xml at 1920x1080 against rtu_render_frame_device of that frame with samples = 1, gather_bounces = 4.

--sorted (alone, or with --sampled / --paths): instead of the comparison with the render, what sorting a shuffled batch on the GPU
buys (tools/sorted_legs.py): the shuffled rays (and keys) (a) as they are, (b) rtu_ray_order_device + gather of rays and keys + the
batch + scatter as one region, (c) those parts one by one, and the image-order batch beside them; every timed launch is complete
(rtu_frame_status) and every sorted one is compared byte for byte with the unsorted answers.

usage: tools/shade_rays_bench.py [--sampled | --paths] [--sorted] [--reps 20] [--warmup 3] [--out FILE]
(profiles/r09_shade_rays.json, r10_shade_rays_sampled.json with --sampled, r12_shade_rays_paths.json with --paths;
profiles/r13_ray_sorting.json collects the --sorted runs of this tool and of tools/ray_query_bench.py)"""
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
PATHS = [("p11_p2_120x68", "Project11/scene.xml"), ("p10_s4_160x120", "Project10/scene.xml")]
SAMPLED = [("p10_s4_160x120", "Project10/scene.xml"), ("p11gs_s2_160x90", "Project11/scene_glossy_soft.xml")]  # (golden holding the scene, its file)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--sampled", action="store_true", help="recipe S: rtu_shade_rays_sampled_device against a one-sample frame")
    ap.add_argument("--paths", action="store_true", help="recipe P: rtu_shade_rays_paths_device against a one-sample frame with gather_bounces = 4")
    ap.add_argument("--sorted", action="store_true", help="time a shuffled batch as it is against order + gather + batch + scatter")
    args = ap.parse_args()
    if args.paths:
        args.sampled = True  # keys, a one-sample frame, 1920x1080: as recipe S
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    pkg = g.load_package()
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)

    def timed(launch, outs):
        """Median / min / max ms of `reps` launches after `warmup` launches; every launch must be complete (rtu_frame_status).
        launch(out) writes to the device tensor `out`: outs[0] while warming up, outs[i % len(outs)] in timed launch i."""
        for _ in range(args.warmup + 8):  # (a capacity report repeats the launch: at most one per recursion level)
            launch(outs[0])
            try:
                ctx.frame_status()
            except pkg.RtuError as err:
                if err.code != pkg.RTU_ERR_CAPACITY:
                    raise
        ms = []
        for i in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch(outs[i % len(outs)])
            e1.record(stream)
            e1.synchronize()
            ctx.frame_status()  # raises if a timed launch was incomplete
            ms.append(e0.elapsed_time(e1))
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    out = {"tool": "shade_rays_bench", "recipe": "P" if args.paths else "S" if args.sampled else "W", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scenes": []}
    for tag, name in (PATHS if args.paths else SAMPLED if args.sampled else [(t, t) for t in TAGS]):
        gd = Golden(tag)
        scene = gd.scene(pkg)
        W, H = (1920, 1080) if args.sampled else (gd.width, gd.height)
        ctx.upload(scene)
        frame = pkg.frame_setup(scene.desc.camera, W, H, samples=1 if args.sampled else 0, gather_bounces=4 if args.paths else 0)
        eye = tuple(frame.cam_pos)
        rays, keys = pkg.camera_sample_rays(frame, 0) if args.sampled else (pkg.camera_rays(frame), None)
        n = rays.size
        if args.sorted:
            from sorted_legs import sorted_legs
            perm = np.random.RandomState(1).permutation(n)
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).to("cuda:0")
            if args.sampled:
                shade = ctx.shade_rays_paths_device if args.paths else ctx.shade_rays_sampled_device
                call = lambda r, k, o: shade(r, k, n, eye, o, stream.cuda_stream)
            else:
                call = lambda r, k, o: ctx.shade_rays_device(r, n, eye, o, stream.cuda_stream)
            row = sorted_legs(pkg, ctx, torch, stream, n, dev(rays), dev(rays[perm]), dev(keys) if args.sampled else None,
                              dev(keys[perm]) if args.sampled else None, 16, call, args.reps, args.warmup, True)
            out["mode"] = "sorted"
            out["scenes"].append(dict(row, scene=name, width=W, height=H))
            continue
        d_out = torch.zeros(n * 4, dtype=torch.float32, device="cuda:0")
        row = {"scene": name, "width": W, "height": H, "rays": int(n), "shade_rays": {}}
        render = timed(lambda o: ctx.render_device(frame, o.data_ptr(), stream.cuda_stream), [d_out])
        render["mrays_per_s"] = n / render["median_ms"] / 1e3
        row["render_frame"] = render
        image = d_out.cpu().numpy().reshape(-1, 4).copy()
        hit = image[:, 3] != np.float32(1.0e30)
        for oname, order in (("image", np.arange(n)), ("shuffled", np.random.RandomState(1).permutation(n))):
            d_rays = torch.from_numpy(np.ascontiguousarray(rays[order]).view(np.uint8).copy()).to("cuda:0")
            d_outs = [torch.zeros(n * 4, dtype=torch.float32, device="cuda:0") for _ in range(args.reps)]  # one per timed launch
            if args.sampled:
                d_keys = torch.from_numpy(keys[order].view(np.int32).copy()).to("cuda:0")
                shade = ctx.shade_rays_paths_device if args.paths else ctx.shade_rays_sampled_device
                t = timed(lambda o: shade(d_rays.data_ptr(), d_keys.data_ptr(), n, eye, o.data_ptr(), stream.cuda_stream), d_outs)
            else:
                t = timed(lambda o: ctx.shade_rays_device(d_rays.data_ptr(), n, eye, o.data_ptr(), stream.cuda_stream), d_outs)
            want = image[order]
            h = hit[order]
            # what is timed is the render's answer, in every timed launch: t at every ray, rgb at every hit ray, bit for bit
            same = True
            for o in d_outs:
                got = o.cpu().numpy().reshape(-1, 4)
                same = same and bool(np.array_equal(got[:, 3].view(np.uint32), want[:, 3].view(np.uint32)) and
                                     np.array_equal(got[h, :3].view(np.uint32), want[h, :3].view(np.uint32)))
            t["equals_render"] = same
            del d_outs
            t["mrays_per_s"] = n / t["median_ms"] / 1e3
            t["ratio_to_render"] = t["median_ms"] / render["median_ms"]
            row["shade_rays"][oname] = t
            del d_rays
        row["hit_rays"] = int(hit.sum())
        out["scenes"].append(row)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
