#!/usr/bin/env python3
"""What temporal gradients cost (rtu_gradient_rays_device, rtu_sample_luminance_device, rtu_temporal_gradient_device,
rtu_temporal_accumulate_gradient_device, rtu_temporal_begin_gradient), one JSON line: Project11 at 1920x1080 as a recipe-P frame of 16
samples. Device figures are medians over `reps` regions bracketed by HIP events on one stream, after `warmup` regions that are not
counted. Needs a GPU.

  kernels   on the last history of the orbit of tools/temporal_bench.py, each against a device copy of the bytes it must read and write
            (P pixels, S = ceil(W / 3) ceil(H / 3) strata):
              rays        40 B written per stratum
              luminance   48 B read + 4 B written per pixel
              gradient    per stratum 4 B (owner) + 64 B (guides) + 64 B (the tap's E, P, N, M) + 4 B (luminance) + 16 B (sample) read,
                          16 B written (k_gradient_diff); 16 B read + 4 B written (k_gradient_lambda, its other taps are its neighbours')
              accumulator the capped form against the moments form on the same inputs, alternating; both read 80 B and write 80 B per
                          pixel besides their taps
  shading   rtu_shade_rays_paths_device of pixels + strata rays against pixels rays, alternating
  session   a frame of a gradient session against a frame of a variance session, alternating: on the orbit, and with the camera at
            rest and the point light moved by rtu_update_scene before every frame (both sessions take rtu_temporal_frame_moved_device
            with an all-STATIC table)
  bench     with --parent-tree DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 320 --warmup 16 in this tree and
            in DIR, alternating, each in a process of its own after this one has closed its context

usage: tools/gradient_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--parent-tree DIR] [--out profiles/r21_gradient.json]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
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
    ap.add_argument("--parent-tree", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    from test_light_lists import RtuLight
    from test_mesh_update_host import clone
    from test_temporal_host import orbit_scene
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("gradient_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    sw, sh = pkg.strata(W, H)
    m = sw * sh
    S = 16
    ctx.upload(scene)
    cams = [pkg.frame_setup(orbit_scene(pkg, scene, k, 60.0, 0.25).desc.camera, W, H, samples=S, gather_bounces=4) for k in range(8)]
    out = {"tool": "gradient_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H, "samples": S, "strata": m, "orbit_step_deg": 0.25}

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

    def alternating(a, b):
        for _ in range(args.warmup):
            a()
            b()
        stream.synchronize()
        a_ms, b_ms = [], []
        for _ in range(args.reps):
            for launch, ms in ((a, a_ms), (b, b_ms)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                launch()
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
        return summary(a_ms), summary(b_ms)

    def copy_ms(nbytes):
        nbytes = max(int(nbytes), 16)
        src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0"), torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
        with torch.cuda.stream(stream):
            return timed(lambda: dst.copy_(src))["median_ms"]

    def floor_ms(read_bytes, written_bytes):
        """A kernel that reads and writes these bytes cannot beat half a copy of each (a copy reads and writes its bytes)."""
        return 0.5 * (copy_ms(read_bytes) + copy_ms(written_bytes))

    # ---- the orbit, accumulated by the entries a gradient session calls -----------------------------------------------------------------
    d_rays = torch.zeros((n + m) * 32, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.zeros(n + m, dtype=torch.int32, device="cuda:0")
    d_img = torch.zeros((n + m, 4), dtype=torch.float32, device="cuda:0")
    d_acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_hist = [torch.zeros(4 * n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    d_lum = [torch.zeros(n, dtype=torch.float32, device="cuda:0") for _ in range(2)]
    d_owner = torch.zeros(m, dtype=torch.int32, device="cuda:0")
    d_diff = torch.zeros((m, 4), dtype=torch.float32, device="cuda:0")
    d_lam = torch.zeros(m, dtype=torch.float32, device="cuda:0")
    motion = np.zeros(scene.desc.n_nodes, pkg.motion_dtype())
    motion["m"], motion["g"], motion["flags"] = np.eye(3, 4, dtype=np.float32), np.eye(3, dtype=np.float32), pkg.RTU_MOTION_STATIC
    d_motion = torch.from_numpy(motion.view(np.uint8).copy()).to("cuda:0")
    desc, gdesc = pkg.temporal_desc(W, H), pkg.gradient_desc(W, H)
    rays_g, keys_g, img_g = d_rays.data_ptr() + 32 * n, d_keys.data_ptr() + 4 * n, d_img.data_ptr() + 16 * n
    torch.cuda.synchronize()

    def shade(count, f):
        for attempt in range(8):  # as a session: shaded again while the frame records did not suffice — and for no other error
            ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), count, tuple(f.cam_pos), d_img.data_ptr(), stream.cuda_stream, max_bounce=f.max_bounce)
            stream.synchronize()
            try:
                ctx.frame_status()
                return
            except pkg.RtuError as err:
                if err.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                    raise

    cur = lcur = 0
    for k, f in enumerate(cams):
        ctx.camera_sample_rays_device(f, k % S, d_rays.data_ptr(), d_keys.data_ptr(), stream.cuda_stream)
        gdesc.frame_index = k
        if k:
            ctx.gradient_rays_device(gdesc, f, (k - 1) % S, rays_g, keys_g, d_owner.data_ptr(), stream.cuda_stream)
        shade(n + m if k else n, f)
        ctx.frame_features_device(f, d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream)
        last = k == len(cams) - 1
        if k:
            ctx.temporal_gradient_device(desc, gdesc, cams[k - 1], f, d_hits.data_ptr(), d_alb.data_ptr(), d_motion.data_ptr(), len(motion),
                                         d_hist[cur].data_ptr(), d_lum[lcur].data_ptr(), d_owner.data_ptr(), img_g, d_diff.data_ptr(), d_lam.data_ptr(),
                                         stream.cuda_stream)
        if not last:  # (the last frame's accumulation and luminance are what is timed below: its inputs stay as they are)
            ctx.temporal_accumulate_gradient_device(desc, cams[k - 1] if k else None, f, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                                    d_hist[cur].data_ptr() if k else None, d_hist[cur ^ 1].data_ptr(), d_acc.data_ptr(), d_motion.data_ptr(),
                                                    len(motion), 0, d_lam.data_ptr() if k else None, stream.cuda_stream)
            ctx.sample_luminance_device(gdesc, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_lum[lcur ^ 1].data_ptr(), stream.cuda_stream)
            cur ^= 1
            lcur ^= 1
    stream.synchronize()
    prev, frame, k_last = cams[-2], cams[-1], len(cams) - 1
    out["lambda_on_the_orbit"] = {"share_above_0": float((d_lam > 0).float().mean().item()), "mean": float(d_lam.mean().item())}

    # ---- the kernels -------------------------------------------------------------------------------------------------------------------
    kernels = {}
    kernels["rays"] = timed(lambda: ctx.gradient_rays_device(gdesc, frame, (k_last - 1) % S, rays_g, keys_g, d_owner.data_ptr(), stream.cuda_stream))
    kernels["rays_floor_ms"] = floor_ms(0, 40 * m)
    kernels["luminance"] = timed(lambda: ctx.sample_luminance_device(gdesc, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_lum[lcur ^ 1].data_ptr(),
                                                                     stream.cuda_stream))
    kernels["luminance_floor_ms"] = floor_ms(48 * n, 4 * n)
    for radius in (0, 1, 3):
        gr = pkg.gradient_desc(W, H, radius=radius, frame_index=k_last)
        kernels["gradient_radius%d" % radius] = timed(lambda: ctx.temporal_gradient_device(
            desc, gr, prev, frame, d_hits.data_ptr(), d_alb.data_ptr(), d_motion.data_ptr(), len(motion), d_hist[cur].data_ptr(), d_lum[lcur].data_ptr(),
            d_owner.data_ptr(), img_g, d_diff.data_ptr(), d_lam.data_ptr(), stream.cuda_stream))
    kernels["gradient_floor_ms"] = floor_ms((152 + 16) * m, (16 + 4) * m)
    ctx.temporal_gradient_device(desc, gdesc, prev, frame, d_hits.data_ptr(), d_alb.data_ptr(), d_motion.data_ptr(), len(motion), d_hist[cur].data_ptr(),
                                 d_lum[lcur].data_ptr(), d_owner.data_ptr(), img_g, d_diff.data_ptr(), d_lam.data_ptr(), stream.cuda_stream)

    def capped():
        ctx.temporal_accumulate_gradient_device(desc, prev, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_hist[cur].data_ptr(),
                                                d_hist[cur ^ 1].data_ptr(), d_acc.data_ptr(), d_motion.data_ptr(), len(motion), 0, d_lam.data_ptr(), stream.cuda_stream)

    def moments():
        ctx.temporal_accumulate_moments_device(desc, prev, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_hist[cur].data_ptr(),
                                               d_hist[2].data_ptr(), d_acc.data_ptr(), d_motion.data_ptr(), len(motion), 0, stream.cuda_stream)
    kernels["accumulator_capped"], kernels["accumulator_moments"] = alternating(capped, moments)
    kernels["accumulator_floor_ms"] = floor_ms(80 * n + 64 * n, 80 * n)
    out["kernels"] = kernels

    # ---- the shading of pixels + strata rays against pixels rays ----------------------------------------------------------------------------
    shade(n + m, frame)  # (and the frame records grown to what the larger batch needs)

    def batch(count):
        return lambda: ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), count, tuple(frame.cam_pos), d_img.data_ptr(), stream.cuda_stream,
                                                   max_bounce=frame.max_bounce)
    both, pixels = alternating(batch(n + m), batch(n))
    stream.synchronize()
    ctx.frame_status()
    out["shading"] = {"pixels_plus_strata": both, "pixels": pixels, "ratio": both["median_ms"] / pixels["median_ms"], "rays_ratio": (n + m) / n}
    del d_hist, d_rays, d_img
    torch.cuda.empty_cache()

    # ---- a gradient session's frame against a variance session's, alternating -----------------------------------------------------------------
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_lam_px = torch.zeros(n, dtype=torch.float32, device="cuda:0")

    def sessions(step):
        a, b = ctx.temporal(desc, variance=pkg.variance_desc(), gradient=pkg.gradient_desc()), ctx.temporal(desc, variance=pkg.variance_desc())
        a_ms, b_ms, share = [], [], []
        for r in range(args.warmup + args.reps):
            call = step(r)
            for s, ms in ((a, a_ms), (b, b_ms)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                call(s)
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            a.lambda_device(d_lam_px.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            share.append(float((d_lam_px > 0).float().mean().item()))
        a.close()
        b.close()
        return {"gradient_frame": summary(a_ms[args.warmup:]), "variance_frame": summary(b_ms[args.warmup:]),
                "gradient_over_variance": statistics.median(a_ms[args.warmup:]) / statistics.median(b_ms[args.warmup:]),
                "mean_share_of_pixels_with_lambda_above_0": statistics.mean(share[args.warmup:])}

    walk = cams + cams[-2:0:-1]  # there and back: 14 steps of 0.25 degrees
    out["session_orbit"] = sessions(lambda r: (lambda s: s.frame_device(walk[r % len(walk)], d_out.data_ptr(), stream.cuda_stream)))

    lights = ctypes.cast(scene.desc.lights, ctypes.POINTER(RtuLight))
    point = [i for i in range(scene.desc.n_lights) if lights[i].type == 2]
    relit = []
    for dx in (0.0, 6.0):
        s2 = clone(pkg, scene)
        l = RtuLight.from_buffer_copy(bytes(ctypes.cast(s2.desc.lights, ctypes.POINTER(RtuLight))[point[0]]))
        l.vec[0] += dx
        s2.set_light(point[0], l)
        relit.append(s2)

    def light_step(r):
        ctx.update(relit[r % 2])  # (not timed: rtu_update_scene is the caller's, and both sessions see it)
        return lambda s: s.frame_moved_device(cams[0], motion, d_out.data_ptr(), 0, stream.cuda_stream)
    out["session_light_moved"] = sessions(light_step)
    ctx.close()
    torch.cuda.empty_cache()

    print(json.dumps(out), file=sys.stderr)  # (kept if the headline below fails)

    # ---- the headline, this tree and the parent's, alternating ------------------------------------------------------------------------
    if args.parent_tree:
        runs = []
        for which, tree in (("this", REPO), ("parent", args.parent_tree)) * 2:
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "320", "--warmup", "16"], cwd=tree, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("gradient_bench: bench.py failed in %s: %s" % (tree, p.stderr[-400:]))
            res = json.loads(p.stdout.strip().splitlines()[-1])
            runs.append({"tree": which, "result": {k: v for k, v in res.items() if not isinstance(v, (dict, list))}})
        out["bench"] = runs
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
