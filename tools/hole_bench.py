#!/usr/bin/env python3
"""What hole rays cost and where (rtu_hole_allocation_device, rtu_hole_fold_device, rtu_temporal_begin_sparse_holes), one JSON line:
Project11 at 1920x1080 as a recipe-P frame of 16 samples, the workload of tools/sparse_bench.py. Device figures are medians over `reps`
regions bracketed by HIP events on one stream, after `warmup` regions that are not counted. Needs a GPU.

  first     frame 0 of a session (after a reset) with the full budget, with budget 0 and of a variance session, alternating, per B
  cut       the four frames after a cut (a jump to a camera 20 degrees on, where it stays) that follows B^2 + 6 frames on the orbit of
            tools/temporal_bench.py, the same three sessions alternating; the hole rays and the holes left to the fill of every frame
  running   a frame of the running session (after min_history B^2 + 6 frames on the orbit walked there and back) with the full
            budget against budget 0, alternating: the allocation and the read-back on a frame with a few thousand holes
  kernels   at B = 2, on the hole plane of frame 0 (every pixel but the owners) and on that of the last orbit frame: the allocation
            entry — a 16-byte memset, k_hole_weight and the three scan kernels of rtu_steer.hip — against the steered allocation on the
            same history and against the copy floor of k_hole_weight alone (1 B read and 4 B written per pixel, 4 B read per hole);
            k_hole_fold against its copy floor (4 B read per pixel; 101 B read and 49 B written per folded hole)
  bench     with --parent-tree DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 320 --warmup 16 in this tree and
            in DIR, alternating, each in a process of its own after this one has closed its context

usage: tools/hole_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--parent-tree DIR] [--out profiles/r23_holes.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
FULL = 1 << 26


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
        raise SystemExit("hole_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    S = 16
    ctx.upload(scene)
    cams = [pkg.frame_setup(orbit_scene(pkg, scene, k, 60.0, 0.25).desc.camera, W, H, samples=S, gather_bounces=4) for k in range(8)]
    cut = pkg.frame_setup(orbit_scene(pkg, scene, 80, 60.0, 0.25).desc.camera, W, H, samples=S, gather_bounces=4)
    walk = cams + cams[-2:0:-1]  # there and back: 14 steps of 0.25 degrees
    out = {"tool": "hole_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H, "samples": S, "orbit_step_deg": 0.25, "pixels": n}
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc()
    min_history = vdesc.min_history
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")

    def timed_frame(s, f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        s.frame_device(f, d_out.data_ptr(), stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    # ---- sessions: frame 0, the frames after a cut, the running session ---------------------------------------------------------------
    sessions = {}
    for B in (2, 3, 4):
        names = ("full", "zero", "variance")
        ss = {"full": ctx.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=B), holes=pkg.hole_desc(budget=FULL)),
              "zero": ctx.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=B), holes=pkg.hole_desc(budget=0)),
              "variance": ctx.temporal(desc, variance=vdesc)}
        first = {k: [] for k in names}
        after = {k: [[] for _ in range(4)] for k in names}
        rays_after, holes_after, rays_first = [], {"full": [], "zero": []}, 0
        lead = B * B + 6
        for r in range(args.warmup + args.reps):
            for k in names:
                ss[k].reset()
            for k in names:
                ms = timed_frame(ss[k], walk[0])
                if r >= args.warmup:
                    first[k].append(ms)
            rays_first = ss["full"].hole_rays()
            for i in range(1, lead):
                for k in names:
                    ss[k].frame_device(walk[i % len(walk)], d_out.data_ptr(), stream.cuda_stream)
            for j in range(4):
                for k in names:
                    ms = timed_frame(ss[k], cut)
                    if r >= args.warmup:
                        after[k][j].append(ms)
                if r == args.warmup:
                    rays_after.append(ss["full"].hole_rays())
                    for k in ("full", "zero"):
                        holes_after[k].append(ss[k].holes())
        # the running session: from frame 0 on the orbit, timed after the settle
        settle = min_history * B * B + 6
        for k in names:
            ss[k].reset()
        run = {k: [] for k in names}
        run_rays, run_holes = [], []
        for r in range(settle + args.reps):
            for k in names:
                ms = timed_frame(ss[k], walk[r % len(walk)])
                if r >= settle:
                    run[k].append(ms)
            if r >= settle:
                run_rays.append(ss["full"].hole_rays())
                run_holes.append(ss["zero"].holes())
        for k in names:
            ss[k].close()
        sessions["B%d" % B] = {
            "frame_0": {k: summary(first[k]) for k in names}, "frame_0_hole_rays": rays_first,
            "lead_frames_before_the_cut": lead,
            "after_cut": {k: [summary(after[k][j]) for j in range(4)] for k in names},
            "after_cut_hole_rays": rays_after, "after_cut_holes_filled": holes_after,
            "settle_frames": settle, "running": {k: summary(run[k]) for k in names},
            "running_full_minus_zero_ms": statistics.median(run["full"]) - statistics.median(run["zero"]),
            "running_hole_rays": [min(run_rays), max(run_rays)], "running_holes_budget_0": [min(run_holes), max(run_holes)]}
    out["sessions"] = sessions

    # ---- the two entries on device memory, B = 2 ---------------------------------------------------------------------------------------
    def timed(launch, before=None):
        ms = []
        for r in range(args.warmup + args.reps):
            if before:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            if r >= args.warmup:
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

    B = 2
    sw, sh = pkg.sparse_blocks(W, H, B)
    m = sw * sh
    sd = pkg.sparse_desc(W, H, block=B)
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_img = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_hist = [torch.zeros(4 * n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    d_owner = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_hole, d_work = torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    d_counts, d_offsets = torch.zeros(n, dtype=torch.int32, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_total = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    d_v = torch.zeros(n, dtype=torch.float32, device="cuda:0")
    motion = np.zeros(scene.desc.n_nodes, pkg.motion_dtype())
    motion["m"], motion["g"], motion["flags"] = np.eye(3, 4, dtype=np.float32), np.eye(3, dtype=np.float32), pkg.RTU_MOTION_STATIC
    d_motion = torch.from_numpy(motion.view(np.uint8).copy()).to("cuda:0")
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

    kernels = {}
    cur = 0
    for k, f in enumerate(cams):  # a sparse chain without hole rays: frame 0 has every hole there is, frame 7 those of a running orbit
        sd.frame_index = k
        ctx.sparse_rays_device(sd, f, d_rays.data_ptr(), d_keys.data_ptr(), d_owner.data_ptr(), stream.cuda_stream)
        shade(m, f)
        ctx.frame_features_device(f, d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream)
        ctx.temporal_accumulate_sparse_device(desc, sd, cams[k - 1] if k else None, f, d_img.data_ptr(), d_owner.data_ptr(), d_hits.data_ptr(),
                                              d_alb.data_ptr(), d_hist[cur].data_ptr() if k else None, d_hist[cur ^ 1].data_ptr(), d_acc.data_ptr(),
                                              d_hole.data_ptr(), d_motion.data_ptr(), len(motion), 0, stream.cuda_stream)
        cur ^= 1
        if k not in (0, len(cams) - 1):
            continue
        stream.synchronize()
        hd = pkg.hole_desc(W, H, budget=FULL, frame_index=k)
        alloc = lambda: ctx.hole_allocation_device(hd, d_hole.data_ptr(), d_hits.data_ptr(), d_counts.data_ptr(), d_offsets.data_ptr(), d_total.data_ptr(),
                                                   stream.cuda_stream)
        st = pkg.steer_desc(W, H, budget=n, max_extra=1, frame_index=k)
        steer = lambda: ctx.sample_allocation_device(st, d_hist[cur].data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), d_counts.data_ptr(), d_offsets.data_ptr(),
                                                     d_total.data_ptr(), stream.cuda_stream)
        kb = {"holes_in_the_plane": int(d_hole.sum().item())}
        kb["steered_allocation"] = timed(steer)
        kb["hole_allocation"] = timed(alloc)
        stream.synchronize()
        total = int(d_total[0].item())
        kb["hole_rays"] = total
        kb["hole_weight_floor_ms"] = floor_ms(n + 4 * kb["holes_in_the_plane"], 4 * n)
        # the fold of `total` samples (whatever d_img holds: finite colours) into copies of the history and of the hole plane
        d_h = d_hist[cur].clone()
        fold = lambda: ctx.hole_fold_device(hd, d_h.data_ptr(), d_acc.data_ptr(), d_work.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_counts.data_ptr(),
                                            d_offsets.data_ptr(), d_img.data_ptr(), min(total, n), stream.cuda_stream)

        def restore():
            with torch.cuda.stream(stream):
                d_work.copy_(d_hole)
        kb["hole_fold"] = timed(fold, restore)
        stream.synchronize()
        kb["folded"] = kb["holes_in_the_plane"] - int(d_work.sum().item())
        kb["hole_fold_floor_ms"] = floor_ms(4 * n + 101 * kb["folded"], 49 * kb["folded"])
        kernels["frame_%d" % k] = kb
        del d_h
    out["kernels_B2"] = kernels
    ctx.close()
    del d_hist, d_rays, d_img
    torch.cuda.empty_cache()

    print(json.dumps(out), file=sys.stderr)  # (kept if the headline below fails)

    # ---- the headline, this tree and the parent's, alternating ------------------------------------------------------------------------
    if args.parent_tree:
        runs = []
        for which, tree in (("this", REPO), ("parent", args.parent_tree)) * 2:
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "320", "--warmup", "16"], cwd=tree, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("hole_bench: bench.py failed in %s: %s" % (tree, p.stderr[-400:]))
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
