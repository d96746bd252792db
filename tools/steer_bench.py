#!/usr/bin/env python3
"""What steered sampling costs (rtu_sample_allocation_device, rtu_extra_sample_rays_device, rtu_temporal_refine_device,
rtu_temporal_begin_steered), one JSON line: Project11 at 1920x1080 as a recipe-P frame of 16 samples on the orbit of
tools/temporal_bench.py. Device figures are medians over `reps` regions bracketed by HIP events on one stream, after `warmup`
regions that are not counted. Needs a GPU.

  kernels   at budgets of 1/4, 1 and 2 rays per pixel (max_extra 3) on the orbit's last history: the allocation (its five launches),
            k_steer_rays and k_refine, each against a device copy of the bytes it must read and write:
              allocation  52 B read (E, M, the first 16 B of the RtuRayHit, v) + 8 B written per pixel
              rays        8 B read per pixel, 40 B written per ray
              fold        8 B read per pixel; per pixel with a count 80 B read + 48 B written; 16 B read per ray
  shading   rtu_shade_rays_paths_device of the extra batch against the same entry on the same number of image-order rays (the first
            `total` rays of the frame's own sample)
  session   a frame of a steered session at each budget against a frame of a variance session, alternating, on the same cameras
  bench     with --parent-tree DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 320 --warmup 16 in this tree and
            in DIR, alternating, each in a process of its own after this one has closed its context

usage: tools/steer_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--parent-tree DIR] [--out profiles/r20_steering.json]"""
import argparse
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
    from test_temporal_host import orbit_scene
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("steer_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    S, E = 16, 3
    ctx.upload(scene)
    cams = [pkg.frame_setup(orbit_scene(pkg, scene, k, 60.0, 0.25).desc.camera, W, H, samples=S, gather_bounces=4) for k in range(8)]
    out = {"tool": "steer_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H, "samples": S, "max_extra": E, "orbit_step_deg": 0.25}

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

    def copy_ms(nbytes):
        nbytes = max(int(nbytes), 16)
        src, dst = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0"), torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
        with torch.cuda.stream(stream):
            return timed(lambda: dst.copy_(src))["median_ms"]

    def floor_ms(read_bytes, written_bytes):
        """A kernel that reads and writes these bytes cannot beat half a copy of each (a copy reads and writes its bytes)."""
        return 0.5 * (copy_ms(read_bytes) + copy_ms(written_bytes))

    # ---- the orbit, accumulated by the entries a variance session calls ------------------------------------------------------------
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_v = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    d_hist = [torch.zeros(4 * n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    motion = np.zeros(scene.desc.n_nodes, pkg.motion_dtype())
    motion["m"], motion["g"], motion["flags"] = np.eye(3, 4, dtype=np.float32), np.eye(3, dtype=np.float32), pkg.RTU_MOTION_STATIC
    d_motion = torch.from_numpy(motion.view(np.uint8).copy()).to("cuda:0")
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    torch.cuda.synchronize()

    def shade(rays_ptr, keys_ptr, count, out_ptr, f):
        for attempt in range(8):  # as a session: shaded again while the frame records did not suffice — and for no other error
            ctx.shade_rays_paths_device(rays_ptr, keys_ptr, count, tuple(f.cam_pos), out_ptr, stream.cuda_stream, max_bounce=f.max_bounce)
            stream.synchronize()
            try:
                ctx.frame_status()
                return
            except pkg.RtuError as err:
                if err.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                    raise

    cur = 0
    for k, f in enumerate(cams):
        ctx.camera_sample_rays_device(f, k % S, d_rays.data_ptr(), d_keys.data_ptr(), stream.cuda_stream)
        shade(d_rays.data_ptr(), d_keys.data_ptr(), n, d_img.data_ptr(), f)
        ctx.frame_features_device(f, d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream)
        ctx.temporal_accumulate_moments_device(desc, cams[k - 1] if k else None, f, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                               d_hist[cur].data_ptr() if k else None, d_hist[cur ^ 1].data_ptr(), d_acc.data_ptr(), d_motion.data_ptr(),
                                               len(motion), 0, stream.cuda_stream)
        cur ^= 1
    hist, frame, k_last = d_hist[cur], cams[-1], len(cams) - 1
    ctx.variance_device(vdesc, hist.data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), stream.cuda_stream)
    stream.synchronize()

    # ---- the three kernels and the extra batch's shading, budget by budget -----------------------------------------------------------
    d_counts = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_offsets = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_total = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    cap = 2 * n
    d_xrays = torch.zeros(cap * 32, dtype=torch.uint8, device="cuda:0")
    d_xkeys = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
    d_owner = torch.zeros(cap, dtype=torch.int32, device="cuda:0")
    d_ximg = torch.zeros((cap, 4), dtype=torch.float32, device="cuda:0")
    scratch_hist = torch.zeros_like(hist)
    scratch_img = torch.zeros_like(d_acc)
    kernels = {}
    for name, budget in (("quarter", n // 4), ("one", n), ("two", 2 * n)):
        sd = pkg.steer_desc(W, H, budget=budget, max_extra=E, frame_index=k_last)
        row = {"budget": budget}
        row["allocation"] = timed(lambda: ctx.sample_allocation_device(sd, hist.data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), d_counts.data_ptr(),
                                                                        d_offsets.data_ptr(), d_total.data_ptr(), stream.cuda_stream))
        stream.synchronize()
        total = int(d_total.item())
        touched = int((d_counts > 0).sum().item())
        row["total"], row["pixels_with_a_count"] = total, touched
        row["allocation_floor_ms"] = floor_ms(52 * n, 8 * n)
        row["rays"] = timed(lambda: ctx.extra_sample_rays_device(sd, frame, d_counts.data_ptr(), d_offsets.data_ptr(), total, d_xrays.data_ptr(),
                                                                 d_xkeys.data_ptr(), d_owner.data_ptr(), stream.cuda_stream))
        row["rays_floor_ms"] = floor_ms(8 * n, 40 * total)
        stream.synchronize()
        shade(d_xrays.data_ptr(), d_xkeys.data_ptr(), total, d_ximg.data_ptr(), frame)  # (and the frame records grown to what it needs)
        row["shade_extra_batch"] = timed(lambda: ctx.shade_rays_paths_device(d_xrays.data_ptr(), d_xkeys.data_ptr(), total, tuple(frame.cam_pos),
                                                                             d_ximg.data_ptr(), stream.cuda_stream, max_bounce=frame.max_bounce))
        stream.synchronize()
        ctx.frame_status()
        if total <= n:
            row["shade_image_order"] = timed(lambda: ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), total, tuple(frame.cam_pos),
                                                                                 d_img.data_ptr(), stream.cuda_stream, max_bounce=frame.max_bounce))
            stream.synchronize()
            ctx.frame_status()
            row["extra_over_image_order"] = row["shade_extra_batch"]["median_ms"] / row["shade_image_order"]["median_ms"]
        shade(d_xrays.data_ptr(), d_xkeys.data_ptr(), total, d_ximg.data_ptr(), frame)

        def fold():  # (on a copy: the fold works in place; the two copies are timed on their own and taken off)
            scratch_hist.copy_(hist)
            scratch_img.copy_(d_acc)
            ctx.temporal_refine_device(desc, scratch_hist.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_counts.data_ptr(), d_offsets.data_ptr(),
                                       d_ximg.data_ptr(), total, scratch_img.data_ptr(), stream.cuda_stream)

        def copies():
            scratch_hist.copy_(hist)
            scratch_img.copy_(d_acc)
        with torch.cuda.stream(stream):
            with_copies, only_copies = timed(fold), timed(copies)
        row["fold_with_its_input_copies"], row["the_input_copies"] = with_copies, only_copies
        row["fold_ms"] = with_copies["median_ms"] - only_copies["median_ms"]
        row["fold_floor_ms"] = floor_ms(8 * n + 80 * touched + 16 * total, 48 * touched)
        kernels[name] = row
    out["kernels"] = kernels

    # ---- a steered session's frame against a variance session's, alternating ------------------------------------------------------------
    walk = cams + cams[-2:0:-1]  # there and back: 14 steps of 0.25 degrees
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    session = {}
    for name, budget in (("quarter", n // 4), ("one", n), ("two", 2 * n)):
        a, b = ctx.temporal(desc, variance=pkg.variance_desc(), steer=pkg.steer_desc(budget=budget, max_extra=E)), ctx.temporal(desc, variance=pkg.variance_desc())
        a_ms, b_ms, totals = [], [], []
        for r in range(args.warmup + args.reps):
            f = walk[r % len(walk)]
            for s, ms in ((a, a_ms), (b, b_ms)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                s.frame_device(f, d_out.data_ptr(), stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            totals.append(a.steer_total())
        a.close()
        b.close()
        session[name] = {"budget": budget, "steered_frame": summary(a_ms[args.warmup:]), "variance_frame": summary(b_ms[args.warmup:]),
                         "mean_total": statistics.mean(totals[args.warmup:]),
                         "steered_over_variance": statistics.median(a_ms[args.warmup:]) / statistics.median(b_ms[args.warmup:])}
    out["session"] = session
    ctx.close()
    del d_xrays, d_ximg, d_hist, scratch_hist
    torch.cuda.empty_cache()

    # ---- the headline, this tree and the parent's, alternating ------------------------------------------------------------------------
    if args.parent_tree:
        runs = []
        for which, tree in (("this", REPO), ("parent", args.parent_tree)) * 2:
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "320", "--warmup", "16"], cwd=tree, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("steer_bench: bench.py failed in %s: %s" % (tree, p.stderr[-400:]))
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
