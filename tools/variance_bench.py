#!/usr/bin/env python3
"""What variance-guided filtering costs (rtu_temporal_accumulate_moments_device, rtu_variance_device, rtu_denoise_variance_device,
rtu_temporal_begin_variance), one JSON line: Project11 at 1920x1080 as a recipe-P frame of 16 samples on the orbit of
tools/temporal_bench.py. Device figures are medians over `reps` regions bracketed by HIP events on one stream, after `warmup`
regions that are not counted. Needs a GPU.

  filter    rtu_denoise_variance_device at 1 .. 5 passes against rtu_denoise_device at the same pass counts, the two alternating pass
            count by pass count in the same run on the same accumulated image, and against a device copy of the bytes the filter must
            read and write (image, hits, albedo, v: 84 B in, 16 B out per pixel). per_pass_ms: the slope between 1 and 5 passes.
  moments   k_temporal_moments against k_temporal_motion on the same buffers (the motion form reads the first three planes of the same
            history), and against its copy floor: 80 B (sample, hit, albedo) + 64 B of taps read where neighbouring lanes share them,
            80 B written per pixel — taken as a copy of 144 B read + 80 B written.
  variance  k_variance with the camera at rest (no short history), on the orbit (short history where surfaces were disoccluded; the share
            is recorded), and with min_history above every history (every lane walks its 49 taps: the worst case); against a copy of
            32 B read (E and M) + 4 B written per pixel — the 16 B of each RtuRayHit it reads at a 48-byte stride are not counted.
  session   a frame of a variance session against a frame of a RTU_TEMPORAL_DENOISE session, alternating, on the same cameras.

usage: tools/variance_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--out profiles/r18_variance.json]"""
import argparse
import json
import os
import statistics
import sys

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
        raise SystemExit("variance_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    S = 16
    ctx.upload(scene)
    cams = [pkg.frame_setup(orbit_scene(pkg, scene, k, 60.0, 0.25).desc.camera, W, H, samples=S, gather_bounces=4) for k in range(8)]
    out = {"tool": "variance_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H, "samples": S, "orbit_step_deg": 0.25}

    def timed(launch):
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
        return summary(ms)

    def copy_ms(nbytes_per_pixel):
        src, dst = torch.zeros(n * nbytes_per_pixel, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * nbytes_per_pixel, dtype=torch.uint8, device="cuda:0")
        with torch.cuda.stream(stream):
            return timed(lambda: dst.copy_(src))

    # ---- real buffers: frames shaded and accumulated by the entries a session calls, at rest and along the orbit --------------------
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_v = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    d_hist = [torch.zeros(4 * n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    motion = np.zeros(scene.desc.n_nodes, pkg.motion_dtype())
    motion["m"], motion["g"], motion["flags"] = np.eye(3, 4, dtype=np.float32), np.eye(3, dtype=np.float32), pkg.RTU_MOTION_STATIC
    d_motion = torch.from_numpy(motion.view(np.uint8).copy()).to("cuda:0")
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    torch.cuda.synchronize()

    def accumulate(frames):
        """The frames one after the other into d_hist[0] / d_hist[1]; returns the index of the last history (its predecessor is the other)."""
        cur = 0
        for k, f in enumerate(frames):
            ctx.camera_sample_rays_device(f, k % S, d_rays.data_ptr(), d_keys.data_ptr(), stream.cuda_stream)
            for attempt in range(8):  # as a session: shaded again while the frame records did not suffice — and for no other error
                ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), n, tuple(f.cam_pos), d_img.data_ptr(), stream.cuda_stream, max_bounce=f.max_bounce)
                stream.synchronize()
                try:
                    ctx.frame_status()
                    break
                except pkg.RtuError as err:
                    if err.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                        raise
            ctx.frame_features_device(f, d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream)
            ctx.temporal_accumulate_moments_device(desc, frames[k - 1] if k else None, f, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                                   d_hist[cur].data_ptr() if k else None, d_hist[cur ^ 1].data_ptr(), d_acc.data_ptr(), d_motion.data_ptr(),
                                                   len(motion), 0, stream.cuda_stream)
            cur ^= 1
        stream.synchronize()
        return cur

    def variance_figures(last):
        nn = d_hist[last][:n * 16].view(torch.float32).reshape(n, 4)[:, 3]
        res = {"short_history_share": float(((nn > 0) & (nn < vdesc.min_history)).float().mean().item()), "mean_history": float(nn.mean().item())}
        res["k_variance"] = timed(lambda: ctx.variance_device(vdesc, d_hist[last].data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), stream.cuda_stream))
        return res

    var = {}
    last = accumulate([cams[0]] * 6)
    var["at_rest"] = variance_figures(last)
    last = accumulate(cams)
    var["orbit"] = variance_figures(last)
    worst = pkg.variance_desc(W, H, min_history=65535)
    var["every_lane_short"] = timed(lambda: ctx.variance_device(worst, d_hist[last].data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), stream.cuda_stream))
    var["copy_32B_per_pixel"], var["copy_4B_per_pixel"] = copy_ms(32), copy_ms(4)
    var["floor_ms"] = 0.5 * (var["copy_32B_per_pixel"]["median_ms"] + var["copy_4B_per_pixel"]["median_ms"])
    out["variance"] = var
    ctx.variance_device(vdesc, d_hist[last].data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), stream.cuda_stream)  # the orbit's v, for the filter
    stream.synchronize()

    # ---- the accumulators on the orbit's last step: previous history d_hist[last ^ 1], cameras cams[-2] -> cams[-1] -----------------
    prev, spare = d_hist[last ^ 1], d_hist[2]
    mom = {"k_temporal_moments": timed(lambda: ctx.temporal_accumulate_moments_device(
        desc, cams[-2], cams[-1], d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), prev.data_ptr(), spare.data_ptr(), d_out.data_ptr(),
        d_motion.data_ptr(), len(motion), 0, stream.cuda_stream))}
    stream.synchronize()
    mom["moments_bytes_equal_the_frame"] = bool(torch.equal(spare, d_hist[last]) and torch.equal(d_out, d_acc))
    mom["k_temporal_motion"] = timed(lambda: ctx.temporal_accumulate_motion_device(
        desc, cams[-2], cams[-1], d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), prev.data_ptr(), spare.data_ptr(), d_out.data_ptr(),
        d_motion.data_ptr(), len(motion), 0, stream.cuda_stream))
    stream.synchronize()
    mom["motion_planes_equal_the_moments_planes"] = bool(torch.equal(spare[:3 * n * 16], d_hist[last][:3 * n * 16]) and torch.equal(d_out, d_acc))
    mom["copy_144B_per_pixel"], mom["copy_80B_per_pixel"] = copy_ms(144), copy_ms(80)
    mom["floor_ms"] = 0.5 * (mom["copy_144B_per_pixel"]["median_ms"] + mom["copy_80B_per_pixel"]["median_ms"])
    mom["moments_over_motion"] = mom["k_temporal_moments"]["median_ms"] / mom["k_temporal_motion"]["median_ms"]
    mom["moments_over_floor"] = mom["k_temporal_moments"]["median_ms"] / mom["floor_ms"]
    out["moments"] = mom

    # ---- the filters on the orbit's accumulated image, pass count by pass count -------------------------------------------------------
    flt = {"passes": {}}
    for p in range(1, 6):
        vd, dd = pkg.variance_desc(W, H, n_passes=p), pkg.denoise_desc(W, H, n_passes=p)
        a = timed(lambda: ctx.denoise_variance_device(vd, d_acc.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_v.data_ptr(), d_out.data_ptr(), stream.cuda_stream))
        b = timed(lambda: ctx.denoise_device(dd, d_acc.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_out.data_ptr(), stream.cuda_stream))
        flt["passes"][str(p)] = {"denoise_variance_device": a, "denoise_device": b, "variance_over_fixed": a["median_ms"] / b["median_ms"]}
    for name in ("denoise_variance_device", "denoise_device"):
        flt[name + "_per_pass_ms"] = (flt["passes"]["5"][name]["median_ms"] - flt["passes"]["1"][name]["median_ms"]) / 4.0
    flt["copy_84B_per_pixel"], flt["copy_16B_per_pixel"] = copy_ms(84), copy_ms(16)
    flt["floor_ms"] = 0.5 * (flt["copy_84B_per_pixel"]["median_ms"] + flt["copy_16B_per_pixel"]["median_ms"])
    flt["defaults_over_floor"] = flt["passes"][str(vdesc.n_passes)]["denoise_variance_device"]["median_ms"] / flt["floor_ms"]
    out["filter"] = flt

    # ---- a variance session's frame against a RTU_TEMPORAL_DENOISE session's, alternating ---------------------------------------------
    walk = cams + cams[-2:0:-1]  # there and back: 14 steps of 0.25 degrees
    a, b = ctx.temporal(desc, variance=pkg.variance_desc()), ctx.temporal(pkg.temporal_desc(W, H, denoise=True))
    a_ms, b_ms = [], []
    for r in range(args.warmup + args.reps):
        f = walk[r % len(walk)]
        for s, ms in ((a, a_ms), (b, b_ms)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            s.frame_device(f, d_out.data_ptr(), stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    a.close()
    b.close()
    out["session"] = {"variance_frame": summary(a_ms[args.warmup:]), "denoise_frame": summary(b_ms[args.warmup:]),
                      "variance_over_denoise": statistics.median(a_ms[args.warmup:]) / statistics.median(b_ms[args.warmup:])}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
