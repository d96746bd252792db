#!/usr/bin/env python3
"""rtu_update_meshes_device against the host path, one JSON line. Per mesh, one animation step = the mesh wobbles
(test_mesh_update_host.deform "wobble", phase k) and its new vertices ARE ALREADY ON THE DEVICE (a torch tensor). In ONE run, alternating
per step:

  * the device path: rtu_update_meshes_device with the tensor's pointer (the reference tree is rebuilt on the GPU);
  * the host path for the same vertices: device-to-host copy + rtu_scene_set_mesh_vertices (bounding box + the reference's BVH build on
    one core) + rtu_update_meshes, on a second context.

Median ms per step by the host clock (every call is synchronous), their spread, and the phase split of both paths from HIP events
(a separate timed run). The baseline of a step is the host path of the same step: no time is fixed in advance, and the tool reports
which way each size falls. Meshes: the teapot (6320 faces), and the teapot with every triangle split in four once and twice (midpoint
subdivision), written as .obj into a temporary directory.

usage: tools/mesh_update_device_bench.py [--reps 15] [--levels 0 1 2] [--out profiles/r28_mesh_update_device.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

WARMUP = 3
XML = """<xml><scene>
  <object type="obj" name="{o}" material="m"></object>
  <object type="plane" name="floor" material="m"><scale value="60"/></object>
  <material type="blinn" name="m"><diffuse r="0.6" g="0.6" b="0.6"/></material>
  <light type="point" name="p"><intensity value="0.7"/><position x="30" y="-40" z="60"/></light>
</scene><camera><position x="0" y="-60" z="30"/><target x="0" y="0" z="8"/><up x="0" y="0" z="1"/><fov value="40"/>
  <width value="320"/><height value="180"/></camera></xml>"""


def subdivide(v, f):
    """Every triangle split in four at its edge midpoints; a midpoint is shared by the two triangles of its edge."""
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    edges, inv = np.unique(e, axis=0, return_inverse=True)
    mid = ((v[edges[:, 0]].astype(np.float64) + v[edges[:, 1]]) * 0.5).astype(np.float32)
    n = len(f)
    m = inv.reshape(-1) + len(v)
    ab, bc, ca = m[:n], m[n:2 * n], m[2 * n:]
    a, b, c = f[:, 0], f[:, 1], f[:, 2]
    nf = np.concatenate([np.stack([a, ab, ca], 1), np.stack([ab, b, bc], 1), np.stack([ca, bc, c], 1), np.stack([ab, bc, ca], 1)])
    return np.concatenate([v, mid]), nf


def write_scene(pkg, d, name, v, f):
    obj = os.path.join(d, name + ".obj")
    with open(obj, "w") as g:
        g.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v.tolist()))
        g.write("".join("f %d %d %d\n" % (t[0] + 1, t[1] + 1, t[2] + 1) for t in f.tolist()))
    xml = os.path.join(d, name + ".xml")
    with open(xml, "w") as g:
        g.write(XML.format(o=obj))
    return pkg.Scene.from_xml(xml)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--levels", type=int, nargs="*", default=[0, 1, 2])
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    from test_mesh_update_host import clone, deform
    pkg = g.load_package()
    teapot = Golden("teapot2_240x135").scene(pkg)
    m = teapot.mesh(0)
    v = teapot.mesh_vertices(0)
    f = np.ctypeslib.as_array(ctypes.cast(m.f, ctypes.POINTER(ctypes.c_uint32)), (m.nf, 3)).astype(np.int64)
    out = {"tool": "mesh_update_device_bench", "reps": args.reps, "warmup": WARMUP, "meshes": []}
    tmp = tempfile.mkdtemp()
    dev, host = pkg.Context(0), pkg.Context(0)
    level = 0
    while level <= max(args.levels):
        if level in args.levels:
            scene = write_scene(pkg, tmp, "teapot%d" % level, v, f)
            mm = scene.mesh(0)
            lo, hi, v0 = list(mm.bound_min), list(mm.bound_max), scene.mesh_vertices(0)
            steps = WARMUP + 2 * args.reps
            held = [torch.from_numpy(deform(v0, lo, hi, "wobble", k)).to("cuda:0") for k in range(steps)]
            torch.cuda.synchronize()
            dev.upload(scene)
            host.upload(scene)
            work = clone(pkg, scene)
            t_dev, t_copy, t_edit, t_upd = [], [], [], []
            for k in range(steps):
                if k == WARMUP + args.reps:  # the second half: the phase split (HIP events; not in the medians)
                    dev.mesh_update_timing(True)
                    host.mesh_update_timing(True)
                    dev.mesh_update_device_timing()
                t0 = time.perf_counter()
                dev.update_meshes_device(scene, {0: (held[k].data_ptr(), None, False)})
                t1 = time.perf_counter()
                vh = held[k].cpu().numpy()
                t2 = time.perf_counter()
                work.set_mesh_vertices(0, vh)
                t3 = time.perf_counter()
                host.update_meshes(work, [0])
                t4 = time.perf_counter()
                if WARMUP <= k < WARMUP + args.reps:
                    t_dev.append((t1 - t0) * 1e3)
                    t_copy.append((t2 - t1) * 1e3)
                    t_edit.append((t3 - t2) * 1e3)
                    t_upd.append((t4 - t3) * 1e3)
            split_dev = {key: val / args.reps for key, val in dev.mesh_update_device_timing().items()}
            split_host = {key: val / args.reps for key, val in host.mesh_update_timing(False).items()}
            dev.mesh_update_timing(False)
            same = all(np.array_equal(dev.mesh_arrays(0)[key].view(np.uint32), host.mesh_arrays(0)[key].view(np.uint32))
                       for key in ("ref_bvh", "ref_elements", "ref_tri", "v"))
            t_host = [a + b + c for a, b, c in zip(t_copy, t_edit, t_upd)]
            d_ms, h_ms = statistics.median(t_dev), statistics.median(t_host)
            h = dev.mesh_shape(0)
            out["meshes"].append({"mesh": "teapot, subdivided %d times" % level, "faces": mm.nf, "vertices": mm.nv, "ref_nodes": h.n_bvh_nodes,
                                  "ref_depth": h.bvh_depth, "device_path_ms": d_ms, "host_path_ms": h_ms,
                                  "host_path_parts_ms": {"device_to_host": statistics.median(t_copy), "set_mesh_vertices": statistics.median(t_edit),
                                                         "update_meshes": statistics.median(t_upd)},
                                  "host_over_device": h_ms / d_ms, "device_path_faster": d_ms < h_ms,
                                  "spread_ms": {"device_path": [min(t_dev), max(t_dev)], "host_path": [min(t_host), max(t_host)]},
                                  "device_phase_ms": split_dev, "host_update_phase_ms": split_host, "same_structures": bool(same)})
            del held
        v, f = subdivide(v, f)
        level += 1
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    dev.close()
    host.close()


if __name__ == "__main__":
    main()
