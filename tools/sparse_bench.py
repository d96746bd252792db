#!/usr/bin/env python3
"""What a sparse session costs and saves (rtu_sparse_rays_device, rtu_temporal_accumulate_sparse_device, rtu_sparse_fill_device,
rtu_temporal_begin_sparse), one JSON line: Project11 at 1920x1080 as a recipe-P frame of 16 samples. Device figures are medians over
`reps` regions bracketed by HIP events on one stream, after `warmup` regions that are not counted. Needs a GPU.

  session   a frame of a sparse session at B = 2, 3, 4 against a frame of a variance session, alternating on the orbit of
            tools/temporal_bench.py walked there and back: `reps` frames of the RUNNING session, after min_history B^2 + 6 frames (a
            pixel's history grows once in B^2 frames; below min_history the variance kernel takes its dearer neighbourhood branch),
            and apart from them the start-up frames before that; the holes of every frame; and the holes of the frames after a cut
            (a jump to a camera 20 degrees on)
  shading   rtu_shade_rays_paths_device of the SW SH rays of a sparse frame against the image's rays, alternating, per B
  kernels   per B, on the last history of the orbit, each against a device copy of the bytes it must read and write (P pixels,
            K = SW SH blocks):
              rays        40 B written per block
              accumulator 64 B (guides) + 64 B (the taps' E, P, N, M) read and 81 B written per pixel, 4 B (owner) + 16 B (sample)
                          read per block; beside it the moments form on an image of samples of the same frame, alternating
              fill        1 B read per pixel; per hole 64 B + up to nine times 20 B + 64 B read and 16 B written: measured on the hole
                          plane of frame 0 (every pixel but its owners is a hole) and on the filled history
  bench     with --parent-tree DIR (a built checkout of the parent commit): bench.py --gpus 1 --steps 320 --warmup 16 in this tree and
            in DIR, alternating, each in a process of its own after this one has closed its context

usage: tools/sparse_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--parent-tree DIR] [--out profiles/r22_sparse.json]"""
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
        raise SystemExit("sparse_bench: no GPU")
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
    out = {"tool": "sparse_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
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

    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_img = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_acc = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_hist = [torch.zeros(4 * n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(3)]
    d_owner = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_hole = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    d_hole0 = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    motion = np.zeros(scene.desc.n_nodes, pkg.motion_dtype())
    motion["m"], motion["g"], motion["flags"] = np.eye(3, 4, dtype=np.float32), np.eye(3, dtype=np.float32), pkg.RTU_MOTION_STATIC
    d_motion = torch.from_numpy(motion.view(np.uint8).copy()).to("cuda:0")
    desc = pkg.temporal_desc(W, H)
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

    shade(n, cams[0])  # (the frame records grown to what the largest batch needs)
    kernels, shading = {}, {}
    for B in (2, 3, 4):
        sw, sh = pkg.sparse_blocks(W, H, B)
        m = sw * sh
        sd = pkg.sparse_desc(W, H, block=B)
        # ---- the orbit, accumulated by the entries a sparse session calls: B * B rounds, so that every pixel has been an owner ----
        walk = [cams[k % len(cams)] if (k // len(cams)) % 2 == 0 else cams[len(cams) - 1 - k % len(cams)] for k in range(max(len(cams), 2 * B * B))]
        cur = 0
        for k, f in enumerate(walk):
            sd.frame_index = k
            ctx.sparse_rays_device(sd, f, d_rays.data_ptr(), d_keys.data_ptr(), d_owner.data_ptr(), stream.cuda_stream)
            shade(m, f)
            ctx.frame_features_device(f, d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream)
            last = k == len(walk) - 1
            if k == 0:  # the hole plane of a frame without history, for the fill's worst case
                ctx.temporal_accumulate_sparse_device(desc, sd, None, f, d_img.data_ptr(), d_owner.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), None,
                                                      d_hist[2].data_ptr(), d_acc.data_ptr(), d_hole0.data_ptr(), d_motion.data_ptr(), len(motion), 0, stream.cuda_stream)
            if not last:  # (the last frame's accumulation is what is timed below: its inputs stay as they are)
                ctx.temporal_accumulate_sparse_device(desc, sd, walk[k - 1] if k else None, f, d_img.data_ptr(), d_owner.data_ptr(), d_hits.data_ptr(),
                                                      d_alb.data_ptr(), d_hist[cur].data_ptr() if k else None, d_hist[cur ^ 1].data_ptr(), d_acc.data_ptr(),
                                                      d_hole.data_ptr(), d_motion.data_ptr(), len(motion), 0, stream.cuda_stream)
                cur ^= 1
        stream.synchronize()
        prev, frame = walk[-2], walk[-1]
        kb = {"blocks": m}
        kb["rays"] = timed(lambda: ctx.sparse_rays_device(sd, frame, d_rays.data_ptr(), d_keys.data_ptr(), d_owner.data_ptr(), stream.cuda_stream))
        kb["rays_floor_ms"] = floor_ms(0, 40 * m)

        def sparse():
            ctx.temporal_accumulate_sparse_device(desc, sd, prev, frame, d_img.data_ptr(), d_owner.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                                  d_hist[cur].data_ptr(), d_hist[cur ^ 1].data_ptr(), d_acc.data_ptr(), d_hole.data_ptr(), d_motion.data_ptr(),
                                                  len(motion), 0, stream.cuda_stream)

        def moments():  # (the image of samples is whatever d_img holds: the same bytes are read)
            ctx.temporal_accumulate_moments_device(desc, prev, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_hist[cur].data_ptr(),
                                                   d_hist[2].data_ptr(), d_acc.data_ptr(), d_motion.data_ptr(), len(motion), 0, stream.cuda_stream)
        kb["accumulator_sparse"], kb["accumulator_moments"] = alternating(sparse, moments)
        kb["accumulator_floor_ms"] = floor_ms(128 * n + 20 * m, 81 * n)
        sparse()
        stream.synchronize()
        kb["holes_filled_history"] = int(d_hole.sum().item())
        kb["holes_frame_0"] = int(d_hole0.sum().item())
        kb["fill_filled_history"] = timed(lambda: ctx.sparse_fill_device(desc, sd, d_hits.data_ptr(), d_alb.data_ptr(), d_owner.data_ptr(), d_img.data_ptr(),
                                                                         d_hole.data_ptr(), d_acc.data_ptr(), stream.cuda_stream))
        kb["fill_frame_0"] = timed(lambda: ctx.sparse_fill_device(desc, sd, d_hits.data_ptr(), d_alb.data_ptr(), d_owner.data_ptr(), d_img.data_ptr(),
                                                                  d_hole0.data_ptr(), d_acc.data_ptr(), stream.cuda_stream))
        kb["fill_floor_filled_history_ms"] = floor_ms(n + 308 * kb["holes_filled_history"], 16 * kb["holes_filled_history"])
        kb["fill_floor_frame_0_ms"] = floor_ms(n + 308 * kb["holes_frame_0"], 16 * kb["holes_frame_0"])
        kernels["B%d" % B] = kb

        # ---- the shading of the blocks' rays against the image's rays ----------------------------------------------------------------
        def batch(count):
            return lambda: ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), count, tuple(frame.cam_pos), d_img.data_ptr(), stream.cuda_stream,
                                                       max_bounce=frame.max_bounce)
        ctx.camera_sample_rays_device(frame, 0, d_rays.data_ptr(), d_keys.data_ptr(), stream.cuda_stream)
        image = timed(batch(n))
        sd.frame_index = len(walk) - 1
        ctx.sparse_rays_device(sd, frame, d_rays.data_ptr(), d_keys.data_ptr(), d_owner.data_ptr(), stream.cuda_stream)
        blocks = timed(batch(m))
        stream.synchronize()
        ctx.frame_status()
        shading["B%d" % B] = {"blocks": blocks, "image": image, "ratio": blocks["median_ms"] / image["median_ms"], "rays_ratio": m / n}
    out["kernels"], out["shading"] = kernels, shading
    del d_hist, d_rays, d_img
    torch.cuda.empty_cache()

    # ---- a sparse session's frame against a variance session's, alternating ----------------------------------------------------------------
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    walk = cams + cams[-2:0:-1]  # there and back: 14 steps of 0.25 degrees
    sessions = {}
    min_history = pkg.variance_desc().min_history
    for B in (2, 3, 4):
        # A pixel is the owner once in B * B frames, so its history reaches the variance kernel's min_history after min_history * B * B
        # frames; until then that kernel takes its neighbourhood branch. The frames before `settle` are the session's start-up (also
        # what follows a reset or a cut) and are reported apart from the running session's.
        settle = min_history * B * B + 6
        a, b = ctx.temporal(desc, variance=pkg.variance_desc(), sparse=pkg.sparse_desc(block=B)), ctx.temporal(desc, variance=pkg.variance_desc())
        a_ms, b_ms, holes = [], [], []
        for r in range(settle + args.reps):
            for s, ms in ((a, a_ms), (b, b_ms)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                s.frame_device(walk[r % len(walk)], d_out.data_ptr(), stream.cuda_stream)
                e1.record(stream)
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            holes.append(a.holes())
        after_cut = []
        for r in range(B * B + 2):  # the camera jumps 20 degrees, then it stays
            a.frame_device(cut, d_out.data_ptr(), stream.cuda_stream)
            after_cut.append(a.holes())
        a.close()
        b.close()
        sessions["B%d" % B] = {"settle_frames": settle, "min_history": min_history,
                               "sparse_frame": summary(a_ms[settle:]), "variance_frame": summary(b_ms[settle:]),
                               "sparse_over_variance": statistics.median(a_ms[settle:]) / statistics.median(b_ms[settle:]),
                               "startup_sparse_frame": summary(a_ms[args.warmup:settle]), "startup_variance_frame": summary(b_ms[args.warmup:settle]),
                               "startup_sparse_ms_per_frame": [round(x, 3) for x in a_ms[:settle]],
                               "holes_per_frame": holes, "holes_after_a_cut": after_cut, "pixels": n}
    out["session_orbit"] = sessions
    ctx.close()
    torch.cuda.empty_cache()

    print(json.dumps(out), file=sys.stderr)  # (kept if the headline below fails)

    # ---- the headline, this tree and the parent's, alternating ------------------------------------------------------------------------
    if args.parent_tree:
        runs = []
        for which, tree in (("this", REPO), ("parent", args.parent_tree)) * 2:
            p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "320", "--warmup", "16"], cwd=tree, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("sparse_bench: bench.py failed in %s: %s" % (tree, p.stderr[-400:]))
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
