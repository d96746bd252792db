#!/usr/bin/env python3
"""What keeping the temporal history across scene updates costs (rtu_scene_motion, rtu_temporal_frame_moved_device,
k_temporal_motion), one JSON line: Project11 at 1920x1080 as a recipe-P frame of 16 samples, the camera at rest, the teapot node
translated a little every frame (there and back). Device figures are medians over `reps` regions bracketed by HIP events on one
stream, after `warmup` regions that are not counted; host figures are medians of the host clock. Needs a GPU.

  animation  per frame, in one loop: rtu_update_scene (host clock, synchronous), rtu_scene_motion (host clock), a moved session's
             frame (rtu_temporal_frame_moved_device, events); and, alternating with it after the same update, a plain session's frame
             (rtu_temporal_frame_device) — the only option without this entry, which starts over. The mean history length of both
             sessions after the last frame.
  kernel     k_temporal_motion (rtu_temporal_accumulate_motion_device) against k_temporal (rtu_temporal_accumulate_device) on the
             same buffers — a rendered sample, its guides and a history of the scene before the step —, alternating, once with the
             camera at rest (k_temporal: one tap everywhere; k_temporal_motion: one tap on still nodes, four on the teapot) and once
             with a moved camera (four taps in both), and against the device-copy floor of tools/temporal_bench.py: a copy of 128 B
             read + 64 B written per pixel.

usage: tools/temporal_motion_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--out profiles/r17_temporal_motion.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

TEAPOT = 7
STEP = 0.05


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
    from test_mesh_update_host import clone
    from test_temporal_host import orbit_scene
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("temporal_motion_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    S = 16
    n_nodes = scene.desc.n_nodes
    scenes = []
    for k in range(8):
        s = clone(pkg, scene)
        s.node_translate(TEAPOT, (STEP * k, 0.0, 0.0))
        scenes.append(s)
    scenes = scenes + scenes[-2:0:-1]  # there and back: 14 steps
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=S, gather_bounces=4)
    out = {"tool": "temporal_motion_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H, "samples": S, "moved_node": TEAPOT, "step": STEP, "n_nodes": n_nodes}
    ctx.upload(scenes[0])
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_n = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def bracket(launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    # ---- the animation: update, table, moved frame — and the plain frame after the same update ------------------------------------
    moved, plain = ctx.temporal(pkg.temporal_desc(W, H)), ctx.temporal(pkg.temporal_desc(W, H))
    still = pkg.scene_motion(scenes[0], scenes[0])
    moved.frame_moved_device(frame, still, d_out.data_ptr(), stream=stream.cuda_stream)
    plain.frame_device(frame, d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    rows = {"update_host_ms": [], "scene_motion_host_ms": [], "frame_moved_ms": [], "frame_plain_ms": [], "frame_moved_host_ms": []}
    for r in range(1, args.warmup + args.reps + 1):
        prev, cur = scenes[(r - 1) % len(scenes)], scenes[r % len(scenes)]
        t0 = time.perf_counter()
        ctx.update(cur)
        t1 = time.perf_counter()
        motion = pkg.scene_motion(prev, cur)
        t2 = time.perf_counter()
        ms_moved = bracket(lambda: moved.frame_moved_device(frame, motion, d_out.data_ptr(), stream=stream.cuda_stream))
        t3 = time.perf_counter()
        ms_plain = bracket(lambda: plain.frame_device(frame, d_out.data_ptr(), stream.cuda_stream))
        for key, v in (("update_host_ms", (t1 - t0) * 1e3), ("scene_motion_host_ms", (t2 - t1) * 1e3), ("frame_moved_ms", ms_moved),
                       ("frame_plain_ms", ms_plain), ("frame_moved_host_ms", (t3 - t2) * 1e3)):
            rows[key].append(v)
    anim = {k: summary(v[args.warmup:]) for k, v in rows.items()}
    anim["per_frame_ms"] = anim["update_host_ms"]["median_ms"] + anim["scene_motion_host_ms"]["median_ms"] + anim["frame_moved_host_ms"]["median_ms"]
    for name, s in (("moved", moved), ("plain", plain)):
        s.history_device(d_n.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        anim["mean_history_" + name] = float(d_n.mean().item())
        anim["max_history_" + name] = float(d_n.max().item())
    moved.close()
    plain.close()
    out["animation"] = anim

    # ---- the kernels on the same buffers ---------------------------------------------------------------------------------------------
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_hist = [torch.zeros(3 * n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    desc = pkg.temporal_desc(W, H)
    other = pkg.frame_setup(orbit_scene(pkg, scene, 1, 60.0, 0.25).desc.camera, W, H, samples=S, gather_bounces=4)
    motion = pkg.scene_motion(scenes[2], scenes[3])
    d_motion = torch.from_numpy(motion.view(np.uint8).copy()).to("cuda:0")

    def sample(sc, k):
        ctx.update(sc)
        ctx.camera_sample_rays_device(frame, k, d_rays.data_ptr(), d_keys.data_ptr(), stream.cuda_stream)
        ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), n, tuple(frame.cam_pos), d_img.data_ptr(), stream.cuda_stream, max_bounce=frame.max_bounce)
        ctx.frame_features_device(frame, d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    sample(scenes[2], 0)  # the history: one frame of the scene before the step
    ctx.temporal_accumulate_device(desc, None, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), None, d_hist[0].data_ptr(), d_out.data_ptr(),
                                   stream.cuda_stream)
    sample(scenes[3], 1)  # the frame: the scene after it
    kern = {}
    for name, prev_cam in (("camera_at_rest", frame), ("camera_moved", other)):
        launches = {
            "k_temporal": lambda: ctx.temporal_accumulate_device(desc, prev_cam, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_hist[0].data_ptr(),
                                                                 d_hist[1].data_ptr(), d_out.data_ptr(), stream.cuda_stream),
            "k_temporal_motion": lambda: ctx.temporal_accumulate_motion_device(desc, prev_cam, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                                                               d_hist[0].data_ptr(), d_hist[1].data_ptr(), d_out.data_ptr(), d_motion.data_ptr(),
                                                                               n_nodes, 0, stream.cuda_stream)}
        ms = {k: [] for k in launches}
        for r in range(args.warmup + args.reps):
            for k, launch in launches.items():  # alternating
                ms[k].append(bracket(launch))
        kern[name] = {k: summary(v[args.warmup:]) for k, v in ms.items()}
        kern[name]["motion_over_plain"] = kern[name]["k_temporal_motion"]["median_ms"] / kern[name]["k_temporal"]["median_ms"]
    src, dst = torch.zeros(n * 128, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 128, dtype=torch.uint8, device="cuda:0")
    c128, c64 = [], []
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.reps):
            c128.append(bracket(lambda: dst.copy_(src)))
            c64.append(bracket(lambda: dst[:n * 64].copy_(src[:n * 64])))
    c128, c64 = summary(c128[args.warmup:]), summary(c64[args.warmup:])
    # a copy of B bytes reads B and writes B: 128 B read + 64 B written is (copy of 128 + copy of 64) / 2
    floor = 0.5 * (c128["median_ms"] + c64["median_ms"])
    kern.update(copy_128B_per_pixel=c128, copy_64B_per_pixel=c64, floor_ms=floor,
                motion_at_rest_over_floor=kern["camera_at_rest"]["k_temporal_motion"]["median_ms"] / floor,
                motion_moved_over_floor=kern["camera_moved"]["k_temporal_motion"]["median_ms"] / floor)
    mv = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    ms = [bracket(lambda: ctx.motion_vectors_device(desc, frame, d_hits.data_ptr(), d_motion.data_ptr(), n_nodes, mv.data_ptr(), stream.cuda_stream))
          for r in range(args.warmup + args.reps)]
    kern["k_motion_vectors"] = summary(ms[args.warmup:])
    out["kernel"] = kern
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
