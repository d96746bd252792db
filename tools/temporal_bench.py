#!/usr/bin/env python3
"""What a temporally accumulated preview costs (rtu_temporal_*, rtu_camera_sample_rays_device), one JSON line: Project11 at 1920x1080
as a recipe-P frame of 16 samples whose camera moves along an orbit, one step per frame. Device figures are medians over `reps`
regions bracketed by HIP events on one stream, after `warmup` regions that are not counted; host figures are medians of the host clock
around synchronous calls. Needs a GPU.

  session   a frame of a session (rtu_temporal_frame_device) with and without RTU_TEMPORAL_DENOISE, and its parts as the session
            calls them, each bracketed on its own: rays (rtu_camera_sample_rays_device), shading (rtu_shade_rays_paths_device),
            guides (rtu_frame_features_device), accumulation (rtu_temporal_accumulate_device), filter (rtu_denoise_device).
  k_temporal  against a device copy of the bytes it must move: 80 B (sample, hit, albedo) + at most 4 x 48 B of taps read — 48 B where
            neighbouring lanes share them — and 64 B written per pixel; the floor is taken as a copy of 128 B read + 64 B written.
  rays      rtu_camera_sample_rays_device against rtu_camera_sample_rays on the host plus the upload of its 36 B per pixel.
  follow    a session frame against the only way to follow a camera without one: rtu_progressive_begin + advance(1) +
            snapshot_denoised + free per camera; the two alternate in the same run, host clock, both synchronous.

usage: tools/temporal_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--out profiles/r16_temporal.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="p11_1080")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    from test_temporal_host import orbit_scene
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    S = 16
    ctx.upload(scene)
    cams = [pkg.frame_setup(orbit_scene(pkg, scene, k, 60.0, 0.25).desc.camera, W, H, samples=S, gather_bounces=4) for k in range(8)]
    cams = cams + cams[-2:0:-1]  # there and back: 14 steps of 0.25 degrees
    out = {"tool": "temporal_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H, "samples": S, "orbit_step_deg": 0.25}
    turn = [0]

    def next_cam():
        turn[0] += 1
        return cams[turn[0] % len(cams)]

    def timed(launch, reps=args.reps):
        for _ in range(args.warmup):
            launch()
        stream.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return summary(ms)

    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    # ---- the session's frame, and its parts ---------------------------------------------------------------------------------------
    ses = {}
    for name, dn in (("frame", False), ("frame_denoised", True)):
        s = ctx.temporal(pkg.temporal_desc(W, H, denoise=dn))
        ses[name] = timed(lambda: s.frame_device(next_cam(), d_out.data_ptr(), stream.cuda_stream))
        d_n = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
        s.history_device(d_n.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        ses[name + "_mean_history"] = float(d_n.mean().item())
        s.close()
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_hist = [torch.zeros(3 * n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    desc = pkg.temporal_desc(W, H)
    torch.cuda.synchronize()
    k = [0]

    def rays():
        k[0] += 1
        ctx.camera_sample_rays_device(cams[k[0] % len(cams)], k[0] % S, d_rays.data_ptr(), d_keys.data_ptr(), stream.cuda_stream)

    def shade():
        f = cams[k[0] % len(cams)]
        ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), n, tuple(f.cam_pos), d_img.data_ptr(), stream.cuda_stream, max_bounce=f.max_bounce)

    def accumulate():
        k[0] += 1
        a, b = d_hist[k[0] & 1], d_hist[(k[0] + 1) & 1]
        ctx.temporal_accumulate_device(desc, cams[(k[0] - 1) % len(cams)], cams[k[0] % len(cams)], d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                       a.data_ptr(), b.data_ptr(), d_out.data_ptr(), stream.cuda_stream)
    parts = {"rays": timed(rays)}
    parts["shading"] = timed(shade)
    try:
        ctx.frame_status()
        parts["shading_complete"] = True
    except pkg.RtuError:  # (the sessions above have grown the frame records: not expected)
        parts["shading_complete"] = False
    parts["guides"] = timed(lambda: ctx.frame_features_device(cams[k[0] % len(cams)], d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream))
    ctx.temporal_accumulate_device(desc, None, cams[k[0] % len(cams)], d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), None, d_hist[k[0] & 1].data_ptr(),
                                   d_out.data_ptr(), stream.cuda_stream)
    parts["accumulation"] = timed(accumulate)
    dd = pkg.denoise_desc(W, H)
    parts["filter"] = timed(lambda: ctx.denoise_device(dd, d_out.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_out.data_ptr(), stream.cuda_stream))
    parts["sum_ms"] = sum(parts[p]["median_ms"] for p in ("rays", "shading", "guides", "accumulation", "filter"))
    ses["parts"] = parts
    out["session"] = ses

    # ---- k_temporal against a copy of its bytes -----------------------------------------------------------------------------------
    src, dst = torch.zeros(n * 128, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 128, dtype=torch.uint8, device="cuda:0")
    with torch.cuda.stream(stream):
        c128 = timed(lambda: dst.copy_(src))
        c64 = timed(lambda: dst[:n * 64].copy_(src[:n * 64]))
    # a copy of B bytes reads B and writes B: 128 B read + 64 B written is (copy of 128 + copy of 64) / 2
    floor = 0.5 * (c128["median_ms"] + c64["median_ms"])
    out["k_temporal"] = {"accumulate_device": parts["accumulation"], "copy_128B_per_pixel": c128, "copy_64B_per_pixel": c64, "floor_ms": floor,
                         "over_floor": parts["accumulation"]["median_ms"] / floor}

    # ---- the ray generator against the host form plus upload ------------------------------------------------------------------------
    ms = []
    for r in range(3):
        f = cams[r]
        t0 = time.perf_counter()
        hr, hk = pkg.camera_sample_rays(f, r)
        t1 = time.perf_counter()
        ctx._check(pkg.hip.rtu_copy_to_device(ctx._h, d_rays.data_ptr(), hr.ctypes.data, 32 * n))
        ctx._check(pkg.hip.rtu_copy_to_device(ctx._h, d_keys.data_ptr(), hk.ctypes.data, 4 * n))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ms.append(((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    host = {"generate_ms": statistics.median(m[0] for m in ms), "upload_ms": statistics.median(m[1] for m in ms)}
    ctx.camera_sample_rays_device(cams[2], 2, d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream)  # (spare buffers of the right sizes)
    stream.synchronize()
    host["device_bytes_equal"] = bool(torch.equal(d_hits[:32 * n], d_rays) and torch.equal(d_alb.view(torch.int32).reshape(-1)[:n], d_keys))
    out["rays"] = {"device": parts["rays"], "host": host, "host_over_device": (host["generate_ms"] + host["upload_ms"]) / parts["rays"]["median_ms"]}

    # ---- following a camera: a session frame against a new progressive session per camera, alternating --------------------------------
    s = ctx.temporal(pkg.temporal_desc(W, H, denoise=True))
    a_ms, b_ms = [], []
    for r in range(args.warmup + args.reps):
        f = next_cam()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.frame_device(f, d_out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        t1 = time.perf_counter()
        p = ctx.progressive(f)
        p.advance(1, stream.cuda_stream)
        p.snapshot_denoised_device(d_out.data_ptr(), None, stream.cuda_stream)
        stream.synchronize()
        p.close()
        t2 = time.perf_counter()
        a_ms.append((t1 - t0) * 1e3)
        b_ms.append((t2 - t1) * 1e3)
    s.close()
    out["follow"] = {"session_frame_host_ms": summary(a_ms[args.warmup:]), "progressive_per_camera_host_ms": summary(b_ms[args.warmup:]),
                     "session_over_progressive": statistics.median(a_ms[args.warmup:]) / statistics.median(b_ms[args.warmup:])}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
