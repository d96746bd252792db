#!/usr/bin/env python3
"""What keeping the temporal history of a DEFORMING mesh costs (rtu_keep_previous_vertices, rtu_scene_motion_deform,
rtu_temporal_frame_deformed_device, rtu_temporal_accumulate_deform_device), one JSON line: Project11 at 1920x1080 as a recipe-P frame of
16 samples, camera at rest, the teapot (mesh 0) wobbling a step further every frame (eight steps there and back).

  animation  per frame, in one loop: rtu_update_meshes (host clock, synchronous), then ALTERNATING the two chains on two sessions of
             the one context — rtu_scene_motion_deform (host clock) + a deformed frame, and rtu_scene_motion with the mesh RESET + a
             moved frame (HIP events on one stream, and the host clock around the call), 24 frames of which the first `warmup`
             are not timed; the mean history over the teapot's pixels of both sessions after the 24th.
  guides     rtu_frame_surface_device against rtu_frame_features_device, alternating.
  kernel     on one set of buffers, alternating: k_temporal_deform with the DEFORM table, k_temporal<true, false> with the RESET table,
             both with an all-STATIC table (a frame with no DEFORM pixel); device copies of the bytes the deform form moves (160 B read,
             64 B written per pixel) as its floor.

usage: tools/deform_temporal_bench.py [--reps 20] [--warmup 4] [--tag p11_1080] [--out profiles/r26_deform_temporal.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

MESH = 0
FRAMES = 24  # of the animation: the history figures are taken after the 24th


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--tag", default="p11_1080")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    from test_mesh_update_host import deformed_scene
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("deform_temporal_bench: no GPU")
    ctx = pkg.Context(0)
    ctx.keep_previous_vertices(True)
    stream = torch.cuda.Stream(device=0)
    gd = Golden(args.tag)
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    n = W * H
    S = 16
    n_nodes = scene.desc.n_nodes
    scenes = [deformed_scene(pkg, scene, MESH, ("wobble", k)) for k in range(8)]
    scenes = scenes + scenes[-2:0:-1]  # there and back: 14 steps
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=S, gather_bounces=4)
    out = {"tool": "deform_temporal_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H, "samples": S, "deformed_mesh": MESH, "n_nodes": n_nodes}
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

    # ---- the animation ----------------------------------------------------------------------------------------------------------------
    deformed, reset = ctx.temporal(pkg.temporal_desc(W, H)), ctx.temporal(pkg.temporal_desc(W, H))
    still = pkg.scene_motion(scenes[0], scenes[0])
    deformed.frame_deformed_device(frame, still, d_out.data_ptr(), stream=stream.cuda_stream)
    reset.frame_moved_device(frame, still, d_out.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    rows = {k: [] for k in ("update_meshes_host_ms", "table_deform_host_ms", "table_reset_host_ms", "frame_deformed_ms", "frame_moved_reset_ms",
                            "frame_deformed_host_ms", "frame_moved_reset_host_ms")}
    for r in range(1, FRAMES + 1):  # (the first `warmup` of them are not counted in the times)
        prev, cur = scenes[(r - 1) % len(scenes)], scenes[r % len(scenes)]
        t0 = time.perf_counter()
        ctx.update_meshes(cur, [MESH])
        t1 = time.perf_counter()
        m_def = pkg.scene_motion(prev, cur, deform_meshes=[MESH])
        t2 = time.perf_counter()
        m_res = pkg.scene_motion(prev, cur, reset_meshes=[MESH])
        t3 = time.perf_counter()
        ms_def = bracket(lambda: deformed.frame_deformed_device(frame, m_def, d_out.data_ptr(), stream=stream.cuda_stream))
        t4 = time.perf_counter()
        ms_res = bracket(lambda: reset.frame_moved_device(frame, m_res, d_out.data_ptr(), stream=stream.cuda_stream))
        t5 = time.perf_counter()
        for key, v in (("update_meshes_host_ms", (t1 - t0) * 1e3), ("table_deform_host_ms", (t2 - t1) * 1e3), ("table_reset_host_ms", (t3 - t2) * 1e3),
                       ("frame_deformed_ms", ms_def), ("frame_moved_reset_ms", ms_res), ("frame_deformed_host_ms", (t4 - t3) * 1e3),
                       ("frame_moved_reset_host_ms", (t5 - t4) * 1e3)):
            rows[key].append(v)
    anim = {k: summary(v[args.warmup:]) for k, v in rows.items()}
    anim["frames"] = FRAMES
    anim["timed_frames"] = FRAMES - args.warmup
    hits, _, surf = ctx.frame_surface(frame)
    on_mesh = torch.from_numpy((surf["mesh"] == MESH).reshape(H, W)).to("cuda:0")
    anim["mesh_pixels"] = int(on_mesh.sum().item())
    for name, s in (("deformed", deformed), ("reset", reset)):
        s.history_device(d_n.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        anim["mean_history_on_mesh_" + name] = float(d_n[on_mesh].mean().item())
        anim["mean_history_" + name] = float(d_n.mean().item())
    anim["deformed_over_reset"] = anim["frame_deformed_ms"]["median_ms"] / anim["frame_moved_reset_ms"]["median_ms"]
    deformed.close()
    reset.close()
    out["animation"] = anim

    # ---- the guides and the kernels on one set of buffers ----------------------------------------------------------------------------
    d_rays = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_keys = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    d_img = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_hits = torch.zeros(n * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.zeros((n, 4), dtype=torch.float32, device="cuda:0")
    d_surf = torch.zeros(n * 32, dtype=torch.uint8, device="cuda:0")
    d_hist = [torch.zeros(3 * n * 16, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    desc = pkg.temporal_desc(W, H)

    def sample(sc, k, upload):
        if upload:
            ctx.upload(sc)
        else:
            ctx.update_meshes(sc, [MESH])
        ctx.camera_sample_rays_device(frame, k, d_rays.data_ptr(), d_keys.data_ptr(), stream.cuda_stream)
        ctx.shade_rays_paths_device(d_rays.data_ptr(), d_keys.data_ptr(), n, tuple(frame.cam_pos), d_img.data_ptr(), stream.cuda_stream, max_bounce=frame.max_bounce)
        ctx.frame_surface_device(frame, d_hits.data_ptr(), d_alb.data_ptr(), d_surf.data_ptr(), stream.cuda_stream)
        stream.synchronize()
    sample(scenes[2], 0, True)  # the history: one frame of the scene before the step
    ctx.temporal_accumulate_device(desc, None, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), None, d_hist[0].data_ptr(), d_out.data_ptr(),
                                   stream.cuda_stream)
    sample(scenes[3], 1, False)  # the frame: the scene after it; the context keeps scenes[2]'s vertices as previous
    guides = {"frame_features_device": [], "frame_surface_device": []}
    d_hits2, d_alb2 = torch.zeros_like(d_hits), torch.zeros_like(d_alb)
    for r in range(args.warmup + args.reps):
        guides["frame_features_device"].append(bracket(lambda: ctx.frame_features_device(frame, d_hits2.data_ptr(), d_alb2.data_ptr(), stream.cuda_stream)))
        guides["frame_surface_device"].append(bracket(lambda: ctx.frame_surface_device(frame, d_hits.data_ptr(), d_alb.data_ptr(), d_surf.data_ptr(),
                                                                                      stream.cuda_stream)))
    out["guides"] = {k: summary(v[args.warmup:]) for k, v in guides.items()}
    out["guides"]["surface_over_features"] = out["guides"]["frame_surface_device"]["median_ms"] / out["guides"]["frame_features_device"]["median_ms"]
    tables = {"deform": pkg.scene_motion(scenes[2], scenes[3], deform_meshes=[MESH]), "reset": pkg.scene_motion(scenes[2], scenes[3], reset_meshes=[MESH]),
              "static": pkg.scene_motion(scenes[3], scenes[3])}
    d_tab = {k: torch.from_numpy(v.view(np.uint8).copy()).to("cuda:0") for k, v in tables.items()}

    def deform(tab):
        return lambda: ctx.temporal_accumulate_deform_device(desc, frame, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_surf.data_ptr(),
                                                             d_hist[0].data_ptr(), d_hist[1].data_ptr(), d_out.data_ptr(), d_tab[tab].data_ptr(), n_nodes, 0,
                                                             stream=stream.cuda_stream)

    def motion(tab):
        return lambda: ctx.temporal_accumulate_motion_device(desc, frame, frame, d_img.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_hist[0].data_ptr(),
                                                             d_hist[1].data_ptr(), d_out.data_ptr(), d_tab[tab].data_ptr(), n_nodes, 0, stream.cuda_stream)
    launches = {"deform_form_deform_table": deform("deform"), "motion_form_reset_table": motion("reset"), "deform_form_static_table": deform("static"),
                "motion_form_static_table": motion("static")}
    ms = {k: [] for k in launches}
    for r in range(args.warmup + args.reps):
        for k, launch in launches.items():  # alternating
            ms[k].append(bracket(launch))
    kern = {k: summary(v[args.warmup:]) for k, v in ms.items()}
    src, dst = torch.zeros(n * 160, dtype=torch.uint8, device="cuda:0"), torch.zeros(n * 160, dtype=torch.uint8, device="cuda:0")
    c160, c64 = [], []
    with torch.cuda.stream(stream):
        for r in range(args.warmup + args.reps):
            c160.append(bracket(lambda: dst.copy_(src)))
            c64.append(bracket(lambda: dst[:n * 64].copy_(src[:n * 64])))
    c160, c64 = summary(c160[args.warmup:]), summary(c64[args.warmup:])
    floor = 0.5 * (c160["median_ms"] + c64["median_ms"])  # a copy of B bytes reads B and writes B
    kern.update(copy_160B_per_pixel=c160, copy_64B_per_pixel=c64, floor_ms=floor,
                deform_over_floor=kern["deform_form_deform_table"]["median_ms"] / floor,
                deform_over_motion_no_deform_pixel=kern["deform_form_static_table"]["median_ms"] / kern["motion_form_static_table"]["median_ms"],
                deform_over_motion_reset=kern["deform_form_deform_table"]["median_ms"] / kern["motion_form_reset_table"]["median_ms"])
    out["kernel"] = kern
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
