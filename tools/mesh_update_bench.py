#!/usr/bin/env python3
"""rtu_update_meshes against rtu_upload_scene, one JSON line. Per scene at 1920x1080, one animation step = the mesh wobbles
(test_mesh_update_host.deform "wobble", phase k):

  * median ms per step of rtu_scene_set_mesh_vertices (host: bounding box + the reference's BVH build), of rtu_update_meshes, and of
    rtu_upload_scene of the SAME deformed scene on a second context in the same run (host clock; all three calls are synchronous).
    The upload is the yardstick: without rtu_update_meshes it is the only way to show a deformed mesh. The tool exits non-zero
    unless edit + update together are faster than the upload;
  * the phase split of an update (HIP events, from a separate timed run): copies, triangle records, refit, placement;
  * the price of the kept topology: ms of a steady-state frame after a refit against the same frame after a fresh upload, for a
    twist of 0, 30, 60 and 120 degrees (rtu_time_render, HIP events around `--frame-iters` frames after warm-up frames).

usage: tools/mesh_update_bench.py [--reps 15] [--out profiles/r07_mesh_update.json]"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SCENES = [("Teapot/scene2", "teapot2_1080"), ("Project13", "p13_200x150")]
WARMUP = 3


def warm_frame(pkg, ctx, frame, d):
    for _ in range(4):  # RTU_ERR_CAPACITY: the context grew its frame records; render again (also learns the launch hints)
        ctx.render_device(frame, d)
        try:
            ctx.frame_status()
        except pkg.RtuError as e:
            if e.code != pkg.RTU_ERR_CAPACITY:
                raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frame-iters", type=int, default=30)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import __graft_entry__ as g
    from conftest import Golden
    from test_mesh_update_host import clone, deform
    pkg = g.load_package()
    upd, fresh = pkg.Context(0), pkg.Context(0)
    out = {"tool": "mesh_update_bench", "reps": args.reps, "warmup": WARMUP, "scenes": []}
    W, H = 1920, 1080
    ok = True
    for name, tag in SCENES:
        scene = Golden(tag).scene(pkg)
        scene.set_resolution(W, H)
        m = scene.mesh(0)
        lo, hi, v0 = list(m.bound_min), list(m.bound_max), scene.mesh_vertices(0)
        frame = pkg.frame_setup(scene.desc.camera, W, H)
        d = pkg.hip.rtu_device_alloc(upd._h, W * H * 16)
        d2 = pkg.hip.rtu_device_alloc(fresh._h, W * H * 16)
        upd.upload(scene)
        work = clone(pkg, scene)
        edit, update, upload = [], [], []
        for k in range(WARMUP + args.reps):
            v = deform(v0, lo, hi, "wobble", k)
            t0 = time.perf_counter()
            work.set_mesh_vertices(0, v)
            t1 = time.perf_counter()
            upd.update_meshes(work, [0])
            t2 = time.perf_counter()
            fresh.upload(work)
            t3 = time.perf_counter()
            if k >= WARMUP:
                edit.append((t1 - t0) * 1e3)
                update.append((t2 - t1) * 1e3)
                upload.append((t3 - t2) * 1e3)
        upd.mesh_update_timing(True)
        for k in range(args.reps):
            work.set_mesh_vertices(0, deform(v0, lo, hi, "wobble", WARMUP + args.reps + k))
            upd.update_meshes(work, [0])
        split = {key: val / args.reps for key, val in upd.mesh_update_timing(False).items()}
        twist = []
        for deg in (0, 30, 60, 120):
            work.set_mesh_vertices(0, deform(v0, lo, hi, "twist", deg))
            upd.upload(scene)  # the topology of the undeformed mesh, then the refit
            upd.update_meshes(work, [0])
            fresh.upload(work)
            row = {"degrees": deg, "ref_nodes": work.mesh(0).n_bvh_nodes}
            for key, ctx, buf in (("refit", upd, d), ("upload", fresh, d2)):
                warm_frame(pkg, ctx, frame, buf)
                row["frame_ms_after_" + key] = statistics.median(ctx.time_render(frame, buf, None, args.frame_iters) for _ in range(3))
            row["ratio"] = row["frame_ms_after_refit"] / row["frame_ms_after_upload"]
            twist.append(row)
        pkg.hip.rtu_device_free(upd._h, d)
        pkg.hip.rtu_device_free(fresh._h, d2)
        e, u, full = statistics.median(edit), statistics.median(update), statistics.median(upload)
        faster = e + u < full
        ok = ok and faster
        out["scenes"].append({"scene": name, "width": W, "height": H, "faces": m.nf, "host_edit_ms": e, "update_meshes_ms": u, "upload_ms": full,
                              "edit_plus_update_ms": e + u, "upload_over_edit_plus_update": full / (e + u), "faster_than_upload": faster,
                              "spread_ms": {"host_edit": [min(edit), max(edit)], "update_meshes": [min(update), max(update)],
                                            "upload": [min(upload), max(upload)]},
                              "update_phase_ms": split, "kept_topology_twist": twist})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    upd.close()
    fresh.close()
    if not ok:
        sys.exit("edit + rtu_update_meshes is not faster than rtu_upload_scene")


if __name__ == "__main__":
    main()
