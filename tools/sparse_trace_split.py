#!/usr/bin/env python3
"""Where the GPU time of a sparse session's frame goes, start-up and running session apart, out of a kernel trace.

  tools/sparse_trace_split.py run B FRAMES         FRAMES frames of a sparse session with block B (0: a variance session) on the orbit of
                                                   tools/sparse_bench.py; run it under  rocprofv3 --kernel-trace --output-format csv -d DIR --
  tools/sparse_trace_split.py split CSV FRAMES SETTLE   the *_kernel_trace.csv of such a run: per kernel the launches per frame and the
                                                   mean ms per frame over frames [1, SETTLE) and [SETTLE, FRAMES). A kernel's launches
                                                   are dealt to the frames in dispatch order, an equal number each; kernels whose
                                                   count is no multiple of FRAMES (set-up work) are listed apart.
Needs a GPU for `run`."""
import csv
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(B, frames):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    from test_temporal_host import orbit_scene
    pkg = g.load_package()
    ctx = pkg.Context(0)
    gd = Golden("p11_1080")
    scene = gd.scene(pkg)
    W, H = gd.width, gd.height
    ctx.upload(scene)
    cams = [pkg.frame_setup(orbit_scene(pkg, scene, k, 60.0, 0.25).desc.camera, W, H, samples=16, gather_bounces=4) for k in range(8)]
    walk = cams + cams[-2:0:-1]
    desc = pkg.temporal_desc(W, H)
    s = ctx.temporal(desc, variance=pkg.variance_desc(), sparse=pkg.sparse_desc(block=B) if B else None)
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream(device=0)
    for r in range(frames):
        s.frame_device(walk[r % len(walk)], d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    s.close()
    ctx.close()


def split(path, frames, settle):
    per = {}
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", ""))
        per.setdefault(name, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    print("# %d frames; start-up: frames 1 .. %d, running: frames %d .. %d; ms per frame" % (frames, settle - 1, settle, frames - 1))
    print("%-44s %9s %10s %10s" % ("kernel", "per frame", "start-up", "running"))
    tot, other = [0.0, 0.0], 0.0
    for name, ms in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        if len(ms) % frames:
            other += sum(ms)
            continue
        c = len(ms) // frames
        a, b = sum(ms[c:c * settle]) / (settle - 1), sum(ms[c * settle:]) / (frames - settle)
        tot[0] += a
        tot[1] += b
        print("%-44s %9d %10.4f %10.4f" % (name[:44], c, a, b))
    print("%-44s %9s %10.4f %10.4f" % ("all of the above", "", tot[0], tot[1]))
    print("# launches that are not per frame (set-up, frame 0's growth): %.3f ms in all" % other)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "run":
        run(int(sys.argv[2]), int(sys.argv[3]))
    elif len(sys.argv) == 5 and sys.argv[1] == "split":
        split(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]))
    else:
        raise SystemExit(__doc__)
