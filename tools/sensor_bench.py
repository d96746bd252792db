#!/usr/bin/env python3
"""Time of a sensor render (rtu_render_sensor_device) against what a caller does today, one JSON line: a 2048x1024 equirectangular
sensor at the golden camera's position on teapot2 (recipe W), Project10/scene.xml (recipe S, 16 samples) and Project11/scene.xml
(recipe P, 16 samples).

  sensor   rtu_render_sensor_device: the rays and keys written on the GPU (k_sensor_rays), the ray-batch launch path, the sums and
           the mean (k_sensor_accumulate). Host clock around the call, which returns when the image is complete; median of `reps`
           after `warmup` calls. Then one more call with rtu_debug_sensor_timing on: the HIP-event time of the two kernels and of
           the whole render, and their share.
  caller   the same image from existing code only, per sample: rtu_sensor_rays on the host, the upload of rays and keys, the
           matching rtu_shade_rays_*_device, rtu_frame_status (a capacity report repeats the launch), a torch sum in sample order;
           then the mean. Host clock around the whole, ending in a synchronise; median of `caller_reps` after one warm-up. Its parts
           (ray generation on the host, upload, shading + status + sum) are reported beside it. The image is compared with the
           sensor's byte for byte (equals_sensor).

usage: tools/sensor_bench.py [--reps 5] [--warmup 2] [--caller-reps 2] [--width 2048] [--height 1024] [--out FILE]
(profiles/r14_sensors.json)"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

# (golden holding the scene, its name, samples, gather_bounces)
WORKLOADS = [("teapot2_1080", "teapot2", 0, 0), ("p10_s4_160x120", "Project10/scene.xml", 16, 0), ("p11_p2_120x68", "Project11/scene.xml", 16, 4)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--caller-reps", type=int, default=2)
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
    W, H = args.width, args.height
    pixels = W * H
    BIG = np.float32(1.0e30)
    out = {"tool": "sensor_bench", "width": W, "height": H, "reps": args.reps, "warmup": args.warmup, "caller_reps": args.caller_reps,
           "device": pkg.device_info(0)["name"], "workloads": []}

    def spread(ms):
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    for tag, name, samples, gather in WORKLOADS:
        scene = Golden(tag).scene(pkg)
        ctx.upload(scene)
        pos, right, up, fwd = camera_basis(scene)
        d = pkg.sensor_desc("equirect", W, H, pos, right, up, fwd, samples=samples, gather_bounces=gather)
        n = max(samples, 1)
        d_img = torch.zeros(pixels * 4, dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()

        def sensor():
            t0 = time.perf_counter()
            ctx.render_sensor_device(d, d_img.data_ptr(), stream.cuda_stream)
            return (time.perf_counter() - t0) * 1e3
        for _ in range(args.warmup):
            sensor()
        row = {"scene": name, "recipe": "P" if gather else "S" if samples else "W", "samples": samples, "rays": pixels * n,
               "sensor": spread([sensor() for _ in range(args.reps)])}
        ctx.sensor_timing(True)
        sensor()
        t = ctx.sensor_timing(False)
        row["kernels"] = {"k_sensor_rays_ms": t["rays"], "k_sensor_accumulate_ms": t["accumulate"], "render_ms": t["render"],
                          "share": (t["rays"] + t["accumulate"]) / t["render"]}
        image = d_img.cpu().numpy().reshape(-1, 4).copy()

        # what a caller does today
        d_out = torch.zeros(pixels * 4, dtype=torch.float32, device="cuda:0")
        shade = ctx.shade_rays_paths_device if gather else ctx.shade_rays_sampled_device

        def caller():
            parts = {"host_rays_ms": 0.0, "upload_ms": 0.0, "shade_status_sum_ms": 0.0}
            t_begin = time.perf_counter()
            with torch.cuda.stream(stream):
                acc = torch.zeros((pixels, 3), dtype=torch.float32, device="cuda:0")
                zs = torch.zeros(pixels, dtype=torch.float32, device="cuda:0")
                nh = torch.zeros(pixels, dtype=torch.int32, device="cuda:0")
                for k in range(n):
                    t0 = time.perf_counter()
                    rays, keys = pkg.sensor_rays(d, k)
                    t1 = time.perf_counter()
                    d_rays = torch.from_numpy(rays.view(np.uint8)).to("cuda:0")
                    d_keys = torch.from_numpy(keys.view(np.int32)).to("cuda:0")
                    stream.synchronize()
                    t2 = time.perf_counter()
                    for attempt in range(16):
                        if samples:
                            shade(d_rays.data_ptr(), d_keys.data_ptr(), pixels, pos, d_out.data_ptr(), stream.cuda_stream)
                        else:
                            ctx.shade_rays_device(d_rays.data_ptr(), pixels, pos, d_out.data_ptr(), stream.cuda_stream)
                        try:
                            ctx.frame_status()
                            break
                        except pkg.RtuError as err:
                            if err.code != pkg.RTU_ERR_CAPACITY:
                                raise
                    o = d_out.view(-1, 4)
                    acc += o[:, :3]
                    hit = (o[:, 3] != float(BIG)) & (o[:, 3] != 0)
                    zs += torch.where(hit, o[:, 3], torch.zeros_like(zs))
                    nh += hit.to(torch.int32)
                    stream.synchronize()
                    t3 = time.perf_counter()
                    parts["host_rays_ms"] += (t1 - t0) * 1e3
                    parts["upload_ms"] += (t2 - t1) * 1e3
                    parts["shade_status_sum_ms"] += (t3 - t2) * 1e3
                img = torch.empty((pixels, 4), dtype=torch.float32, device="cuda:0")
                img[:, :3] = acc / float(n)
                img[:, 3] = torch.where(nh > 0, zs / nh.to(torch.float32), torch.full_like(zs, float(BIG)))
                stream.synchronize()
            return (time.perf_counter() - t_begin) * 1e3, parts, img
        caller()
        runs = [caller() for _ in range(args.caller_reps)]
        row["caller"] = spread([r[0] for r in runs])
        row["caller"]["parts_of_last_run"] = runs[-1][1]
        row["caller"]["equals_sensor"] = bool(np.array_equal(runs[-1][2].cpu().numpy().view(np.uint32), image.view(np.uint32)))
        row["caller_over_sensor"] = row["caller"]["median_ms"] / row["sensor"]["median_ms"]
        row["hit_pixels"] = int((image[:, 3] != BIG).sum())
        out["workloads"].append(row)
        del d_img, d_out
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
