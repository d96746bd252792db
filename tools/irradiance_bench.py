#!/usr/bin/env python3
"""What the irradiance map costs and what it buys (rtu_irradiance_build, rtu_render_frame_irradiance), one JSON line: Project11 at
1920x1080.

  build     rtu_irradiance_build_device at the defaults (min_subdiv -5, max_subdiv 0, 64 samples per computed point, thresholds
            1e30 / 1e30 / 0.7): wall time (the call reads a list length back per pass), and the share of points computed per pass
  frames    the irradiance frame at 16 samples, a recipe-P frame at 64 samples and a recipe-P frame whose sample count makes it cost
            what build + irradiance frame cost, ALTERNATING region by region in one run (wall time around synchronous calls)
  halves    rtu_gather_rays_device against rtu_shade_rays_paths_device and rtu_shade_rays_ambient_device against
            rtu_shade_rays_sampled_device on one sample's rays of the frame, alternating, bracketed by HIP events
  lookup    rtu_irradiance_sample_device at every pixel centre against a device copy of the 40 bytes per position it moves
  error     root-mean-square difference (linear rgb, pixels whose every sample hit) of the three images from a 1024-sample recipe-P
            frame rendered on the device

usage: tools/irradiance_bench.py [--reps 5] [--warmup 1] [--tag p11_1080] [--ref-samples 1024] [--out profiles/r27_irradiance.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--tag", default="p11_1080")
    ap.add_argument("--ref-samples", type=int, default=1024)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("irradiance_bench: no GPU")
    ctx = pkg.Context(0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    ctx.upload(scene)
    out = {"tool": "irradiance_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "tag": args.tag,
           "width": W, "height": H}

    def stats(v):
        return {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v)}

    def wall(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    # ---- build ----
    desc = pkg.irradiance_desc()
    gw, gh, passes = pkg.irradiance_grid(desc, W, H)
    d_rec = torch.zeros(gw * gh * 8, dtype=torch.float32, device="cuda:0")
    d_comp = torch.zeros(gw * gh, dtype=torch.uint8, device="cuda:0")
    frame0 = pkg.frame_setup(scene.desc.camera, W, H)
    per = None
    ms = []
    for i in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        per = ctx.irradiance_build_device(frame0, desc, d_rec.data_ptr(), d_comp.data_ptr())
        t = (time.perf_counter() - t0) * 1e3
        if i >= args.warmup:
            ms.append(t)
    out["build"] = dict(stats(ms), grid=[gw, gh], samples=desc.samples, points=gw * gh, computed=int(per[:, 1].sum()),
                        computed_share=float(per[:, 1].sum()) / (gw * gh),
                        passes=[{"visited": int(v), "computed": int(c), "share": (float(c) / float(v) if v else 0.0)} for v, c in per])
    build_ms = out["build"]["median_ms"]

    # ---- frames ----
    d_img = [torch.zeros(n * 4, dtype=torch.float32, device="cuda:0") for _ in range(3)]
    f_irr = pkg.frame_setup(scene.desc.camera, W, H, samples=16)
    f_p64 = pkg.frame_setup(scene.desc.camera, W, H, samples=64, gather_bounces=4)
    irr_once = wall(lambda: ctx.render_irradiance_device(f_irr, d_rec.data_ptr(), desc.max_subdiv, d_img[0].data_ptr()))
    irr_once = wall(lambda: ctx.render_irradiance_device(f_irr, d_rec.data_ptr(), desc.max_subdiv, d_img[0].data_ptr()))
    p64_once = wall(lambda: ctx.render_device(f_p64, d_img[1].data_ptr()))
    p64_once = wall(lambda: ctx.render_device(f_p64, d_img[1].data_ptr()))
    eq = max(1, int(round(64.0 * (build_ms + irr_once) / p64_once)))
    f_peq = pkg.frame_setup(scene.desc.camera, W, H, samples=eq, gather_bounces=4)
    launches = {
        "irradiance_frame_16": lambda: ctx.render_irradiance_device(f_irr, d_rec.data_ptr(), desc.max_subdiv, d_img[0].data_ptr()),
        "recipe_p_64": lambda: ctx.render_device(f_p64, d_img[1].data_ptr()),
        "recipe_p_equal_time": lambda: ctx.render_device(f_peq, d_img[2].data_ptr()),
    }
    for _ in range(args.warmup):
        for f in launches.values():
            wall(f)
    ms = {k: [] for k in launches}
    for _ in range(args.reps):
        for k, f in launches.items():
            ms[k].append(wall(f))
    out["frames"] = {k: stats(v) for k, v in ms.items()}
    out["frames"]["equal_time_samples"] = eq
    out["frames"]["build_plus_irradiance_frame_ms"] = build_ms + out["frames"]["irradiance_frame_16"]["median_ms"]

    # ---- error against a long recipe-P frame ----
    f_ref = pkg.frame_setup(scene.desc.camera, W, H, samples=args.ref_samples, gather_bounces=4)
    d_ref = torch.zeros(n * 4, dtype=torch.float32, device="cuda:0")
    ref_ms = wall(lambda: ctx.render_device(f_ref, d_ref.data_ptr()))
    ref = d_ref.cpu().numpy().reshape(-1, 4)
    imgs = [d.cpu().numpy().reshape(-1, 4) for d in d_img]
    solid = (ref[:, 3] < 1e29) & np.isfinite(ref[:, :3]).all(axis=1)
    for im in imgs:
        solid &= np.isfinite(im[:, :3]).all(axis=1)
    out["error"] = {"reference_samples": args.ref_samples, "reference_ms": ref_ms, "pixels": int(solid.sum())}
    for name, im in zip(launches, imgs):
        d = im[solid, :3].astype(np.float64) - ref[solid, :3].astype(np.float64)
        out["error"][name] = {"rmse": float(np.sqrt((d * d).mean())), "mean_signed": float(d.mean())}

    # ---- the halves, and the lookup ----
    stream = torch.cuda.Stream(device=0)
    s = stream.cuda_stream
    rays, keys = pkg.camera_sample_rays(f_irr, 0)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to("cuda:0")
    d_keys = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32).copy()).to("cuda:0")
    d_o = [torch.zeros(n * 4, dtype=torch.float32, device="cuda:0") for _ in range(4)]
    centres = np.stack(np.meshgrid(np.arange(W, dtype=np.float32) + 0.5, np.arange(H, dtype=np.float32) + 0.5), axis=-1).reshape(-1, 2)
    d_xy = torch.from_numpy(np.ascontiguousarray(centres)).to("cuda:0")
    d_look = torch.zeros(n * 8, dtype=torch.float32, device="cuda:0")
    d_src, d_dst = torch.zeros(n * 10, dtype=torch.float32, device="cuda:0"), torch.zeros(n * 10, dtype=torch.float32, device="cuda:0")
    eye = tuple(f_irr.cam_pos)
    torch.cuda.synchronize()
    half = {
        "shade_rays_paths_device": lambda: ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), n, eye, d_o[0].data_ptr(), s),
        "gather_rays_device": lambda: ctx.gather_rays_device(d_rays.data_ptr(), d_keys.data_ptr(), n, eye, d_o[1].data_ptr(), s),
        "shade_rays_sampled_device": lambda: ctx.shade_rays_sampled_device(d_rays.data_ptr(), d_keys.data_ptr(), n, eye, d_o[2].data_ptr(), s),
        "shade_rays_ambient_device": lambda: ctx.shade_rays_ambient_device(d_rays.data_ptr(), d_keys.data_ptr(), d_o[1].data_ptr(), n, eye, d_o[3].data_ptr(), s),
        "irradiance_sample_device": lambda: ctx.irradiance_sample_device(d_rec.data_ptr(), W, H, desc.max_subdiv, d_xy.data_ptr(), n, d_look.data_ptr(), s),
        "copy_40B_per_position": lambda: d_dst.copy_(d_src, non_blocking=True),
    }
    with torch.cuda.stream(stream):
        for _ in range(args.warmup + 1):
            for f in half.values():
                f()
        stream.synchronize()
        ctx.frame_status()
        ms = {k: [] for k in half}
        for _ in range(args.reps):
            for k, f in half.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                f()
                e1.record(stream)
                e1.synchronize()
                ms[k].append(e0.elapsed_time(e1))
    ctx.frame_status()
    out["halves"] = {k: stats(v) for k, v in ms.items()}
    out["halves"]["ambient_of_gather_equals_paths"] = bool(torch.equal(d_o[0].view(torch.int32), d_o[3].view(torch.int32)))
    ctx.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(os.path.join(REPO, args.out) if not os.path.isabs(args.out) else args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
