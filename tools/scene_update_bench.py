#!/usr/bin/env python3
"""rtu_update_scene against rtu_upload_scene, one JSON line: per scene at 1920x1080 the median milliseconds of an upload, of an
update for one animation step (the first shadow light orbits, the first mesh node turns), the split of an update's device builder
into its phases (HIP events, from a separate timed run: timing synchronises between phases), and the time of the first frame
rendered after an update (host clock around rtu_render_frame_device + rtu_frame_status).

usage: tools/scene_update_bench.py [--reps 15] [--out profiles/r05_scene_update.json]"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

SCENES = [("Teapot/scene2", "teapot2_1080"), ("Project13", "p13_200x150")]


def step(pkg, scene, i):
    from test_light_lists import RtuLight, RtuNode
    d = scene.desc
    lights = ctypes.cast(d.lights, ctypes.POINTER(RtuLight))
    nodes = ctypes.cast(d.nodes, ctypes.POINTER(RtuNode))
    sl = [k for k in range(d.n_lights) if lights[k].type != 0][0]
    nl = RtuLight.from_buffer_copy(bytes(lights[sl]))
    a = 0.05 * (i + 1)
    if nl.type == 2:
        r = math.hypot(nl.vec[0], nl.vec[1]) or 10.0
        nl.vec[0], nl.vec[1] = r * math.cos(a), r * math.sin(a)
    else:
        nl.vec[0], nl.vec[1], nl.vec[2] = math.cos(a), math.sin(a), -0.8
    scene.set_light(sl, nl)
    mesh = [k for k in range(d.n_nodes) if nodes[k].obj_type == 3][0]
    scene.node_rotate(mesh, (0.0, 0.0, 1.0), 3.0)


def render(pkg, ctx, frame, d):
    for _ in range(3):  # RTU_ERR_CAPACITY: the context grew its frame records; render again
        ctx.render_device(frame, d)
        try:
            ctx.frame_status()
            return
        except pkg.RtuError as e:
            if e.code != pkg.RTU_ERR_CAPACITY:
                raise


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import __graft_entry__ as g
    from conftest import Golden
    pkg = g.load_package()
    ctx = pkg.Context(0)
    out = {"tool": "scene_update_bench", "reps": args.reps, "scenes": []}
    W, H = 1920, 1080
    for name, tag in SCENES:
        scene = Golden(tag).scene(pkg)
        scene.set_resolution(W, H)
        frame = pkg.frame_setup(scene.desc.camera, W, H)
        d = pkg.hip.rtu_device_alloc(ctx._h, W * H * 16)
        up = []
        for _ in range(max(3, args.reps // 3)):
            t0 = time.perf_counter()
            ctx.upload(scene)
            up.append((time.perf_counter() - t0) * 1e3)
        render(pkg, ctx, frame, d)
        upd, first = [], []
        for i in range(args.reps):
            step(pkg, scene, i)
            t0 = time.perf_counter()
            ctx.update(scene)
            t1 = time.perf_counter()
            render(pkg, ctx, frame, d)
            t2 = time.perf_counter()
            upd.append((t1 - t0) * 1e3)
            first.append((t2 - t1) * 1e3)
        ctx.update_timing(True)
        for i in range(args.reps):
            step(pkg, scene, args.reps + i)
            ctx.update(scene)
        split = {k: v / args.reps for k, v in ctx.update_timing(False).items()}
        pkg.hip.rtu_device_free(ctx._h, d)
        out["scenes"].append({"scene": name, "width": W, "height": H, "upload_ms": statistics.median(up), "update_ms": statistics.median(upd),
                              "update_phase_ms": split, "first_frame_after_update_ms": statistics.median(first),
                              "lists": ctx.light_lists()})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
