#!/usr/bin/env python3
"""What a denoised preview costs (rtu_frame_features_device, rtu_denoise_device, rtu_progressive_snapshot_denoised_device), one JSON
line: Project11 at 1920x1080 as a recipe-P frame. Every figure but the progressive pass is the median over `reps` regions bracketed by
HIP events on one stream, after `warmup` regions that are not counted; the pass (rtu_progressive_advance, synchronous) is timed on
the host clock.

  features   rtu_frame_features_device against rtu_trace_rays_device and rtu_ray_features_device on the uploaded rtu_camera_rays of the
             same frame: what the albedo and what generating the rays in the kernel cost. The three answers are compared.
  denoise    rtu_denoise_device of a 1-sample snapshot with n_passes = 1 .. 5: the totals, and their differences as the cost of each
             pass (the first figure includes the plane-making kernel); against a torch restatement of the same filter on the GPU — what a
             user does by hand today —, whose output is compared word by word; and against a device copy of the bytes the filter must
             read and write (80 B in, 16 B out per pixel), as the floor.
  preview    rtu_progressive_snapshot_denoised_device against rtu_progressive_snapshot_device and against the 1-sample pass it cleans.

usage: tools/denoise_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--out profiles/r15_denoise.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


def torch_denoise(torch, rgbz, flags, t, P, N, albedo, desc):
    """The rules of include/rtu_render.h ("Denoising") on whole tensors with shifted views, one tap at a time in the rules' order.
    rgbz [H, W, 4], flags int32 [H, W], t [H, W], P, N [H, W, 3], albedo [H, W, 4]: float32 tensors on one device."""
    H, W = rgbz.shape[:2]
    one = torch.ones((), dtype=torch.float32, device=rgbz.device)
    zero = torch.zeros((), dtype=torch.float32, device=rgbz.device)
    k = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]

    def dot3(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    c = rgbz[..., :3]
    valid = (flags & 1) != 0
    a = albedo[..., :3]
    d = torch.where(a > 0.01, a, one)
    den = desc.sigma_plane * t
    e = c / d
    for i in range(desc.n_passes):
        s = 1 << i
        sc = torch.tensor(desc.sigma_color, dtype=torch.float32) * torch.tensor(2.0 ** -i, dtype=torch.float32)
        sc2 = float(sc * sc)
        acc = torch.zeros((H, W, 3), dtype=torch.float32, device=rgbz.device)
        wsum = torch.zeros((H, W), dtype=torch.float32, device=rgbz.device)
        for dy in range(-2, 3):
            for dx in range(-2, 3):
                y0, y1, x0, x1 = max(0, -dy * s), min(H, H - dy * s), max(0, -dx * s), min(W, W - dx * s)
                if y0 >= y1 or x0 >= x1:
                    continue
                ps = (slice(y0, y1), slice(x0, x1))
                qs = (slice(y0 + dy * s, y1 + dy * s), slice(x0 + dx * s, x1 + dx * s))
                h = k[dy + 2] * k[dx + 2]
                dot = dot3(N[ps], N[qs])
                w = torch.where(dot > 0, dot, zero)
                for _ in range(desc.normal_log2_power):
                    w = w * w
                x = dot3(N[ps], P[qs] - P[ps]) / den[ps]
                wp = 1.0 / (1.0 + x * x)
                dl = e[qs] - e[ps]
                wc = 1.0 / (1.0 + dot3(dl, dl) / sc2)
                w = ((h * w) * wp) * wc
                m = valid[qs]
                acc[ps] = torch.where(m[..., None], acc[ps] + e[qs] * w[..., None], acc[ps])
                wsum[ps] = torch.where(m, wsum[ps] + w, wsum[ps])
        upd = valid & (wsum > 0)
        e = torch.where(upd[..., None], acc / wsum[..., None], e)
    out = rgbz.clone()
    out[..., :3] = torch.where(valid[..., None], e * d, c)
    return out


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
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("denoise_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    ctx.upload(scene)
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=4, gather_bounces=4)
    out = {"tool": "denoise_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H}

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
        return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}

    # ---- features -----------------------------------------------------------------------------------------------------------------
    rays = pkg.camera_rays(frame)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to("cuda:0")
    d_hits = [torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    d_alb = [torch.zeros((n, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    feat = {
        "trace_rays_device": timed(lambda: ctx.trace_rays_device(d_rays.data_ptr(), n, d_hits[0].data_ptr(), stream.cuda_stream)),
        "ray_features_device": timed(lambda: ctx.ray_features_device(d_rays.data_ptr(), n, d_hits[1].data_ptr(), d_alb[0].data_ptr(), stream.cuda_stream)),
        "frame_features_device": timed(lambda: ctx.frame_features_device(frame, d_hits[2].data_ptr(), d_alb[1].data_ptr(), stream.cuda_stream)),
    }
    feat["hits_equal"] = bool(torch.equal(d_hits[0], d_hits[1]) and torch.equal(d_hits[0], d_hits[2]))
    feat["albedo_equal"] = bool(torch.equal(d_alb[0].view(torch.int32), d_alb[1].view(torch.int32)))
    feat["albedo_over_trace"] = feat["ray_features_device"]["median_ms"] / feat["trace_rays_device"]["median_ms"]
    feat["frame_over_trace"] = feat["frame_features_device"]["median_ms"] / feat["trace_rays_device"]["median_ms"]
    out["features"] = feat

    # ---- the filter on a 1-sample snapshot ----------------------------------------------------------------------------------------
    session = ctx.progressive(frame)
    session.advance(1)
    d_img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    session.snapshot_device(d_img.data_ptr(), None, stream.cuda_stream)
    stream.synchronize()
    hits_t, alb_t = d_hits[2], d_alb[1]
    den = {}
    for k in range(1, 6):
        desc = pkg.denoise_desc(W, H, n_passes=k)
        den["n_passes_%d" % k] = timed(lambda: ctx.denoise_device(desc, d_img.data_ptr(), hits_t.data_ptr(), alb_t.data_ptr(), d_out.data_ptr(), stream.cuda_stream))
    den["per_pass_ms"] = [den["n_passes_1"]["median_ms"]] + [den["n_passes_%d" % k]["median_ms"] - den["n_passes_%d" % (k - 1)]["median_ms"] for k in range(2, 6)]
    total = den["n_passes_5"]["median_ms"]
    # the floor: a device copy of the bytes the filter has to read (image, hits, albedo: 80 B per pixel) and write (16 B per pixel)
    src, dst = torch.zeros(n * 80, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 80, dtype=torch.uint8, device="cuda:0")
    with torch.cuda.stream(stream):
        den["copy_80B_per_pixel"] = timed(lambda: dst.copy_(src))
        den["copy_16B_per_pixel"] = timed(lambda: dst[:n * 16].copy_(src[:n * 16]))
        hv = hits_t.view(torch.float32).view(H, W, 12)
        flags_t = hits_t.view(torch.int32).view(H, W, 12)[..., 2].contiguous()
        t_t, P_t, N_t = hv[..., 0].contiguous(), hv[..., 4:7].contiguous(), hv[..., 8:11].contiguous()
        alb_hw = alb_t.view(H, W, 4)
        desc = pkg.denoise_desc(W, H)
        result = [None]

        def by_hand():
            result[0] = torch_denoise(torch, d_img, flags_t, t_t, P_t, N_t, alb_hw, desc)
        den["torch_restatement"] = timed(by_hand, reps=max(3, args.reps // 4))
        stream.synchronize()
        ours, theirs = d_out, result[0]  # d_out: the 5-pass run above
        words = (ours.view(torch.int32) != theirs.view(torch.int32))
        den["torch_words_differ"] = int(words.sum().item())
        den["torch_max_abs_diff"] = float((ours - theirs).abs().nan_to_num(0.0).max().item())
    den["floor_ms"] = den["copy_80B_per_pixel"]["median_ms"] * 0.5 + den["copy_16B_per_pixel"]["median_ms"] * 0.5
    den["total_over_floor"] = total / den["floor_ms"]
    den["torch_over_total"] = den["torch_restatement"]["median_ms"] / total
    out["denoise"] = den

    # ---- the preview: a denoised snapshot against the pass it cleans ------------------------------------------------------------------
    prev = {"snapshot_device": timed(lambda: session.snapshot_device(d_out.data_ptr(), None, stream.cuda_stream)),
            "snapshot_denoised_device": timed(lambda: session.snapshot_denoised_device(d_out.data_ptr(), None, stream.cuda_stream))}
    session.close()
    ms = []
    for r in range(args.warmup + max(3, args.reps // 4)):
        s = ctx.progressive(frame)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.advance(1)  # synchronous
        ms.append((time.perf_counter() - t0) * 1e3)
        s.close()
    ms = ms[args.warmup:]
    prev["advance_1_sample_host_ms"] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}
    prev["denoised_snapshot_over_pass"] = prev["snapshot_denoised_device"]["median_ms"] / prev["advance_1_sample_host_ms"]["median_ms"]
    prev["filter_over_pass"] = total / prev["advance_1_sample_host_ms"]["median_ms"]
    out["preview"] = prev
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
