#!/usr/bin/env python3
"""Where the GPU time of a frame with hole rays goes, out of a kernel trace of the running session.

  tools/hole_trace_split.py run B BUDGET FRAMES          FRAMES frames of a sparse session with block B and hole rays of BUDGET (0: none) on
                                                         the orbit of tools/hole_bench.py; run it under
                                                         rocprofv3 --kernel-trace --output-format csv -d DIR --
  tools/hole_trace_split.py split CSV FRAMES SETTLE [CSV0]   the *_kernel_trace.csv of such a run: per kernel the launches and the mean ms
                                                         per frame over frames [SETTLE, FRAMES). A frame begins at its k_sparse_rays
                                                         dispatch. With CSV0, the trace of a BUDGET 0 run, its column stands beside.
Needs a GPU for `run`."""
import csv
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(B, budget, frames):
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
    s = ctx.temporal(pkg.temporal_desc(W, H), variance=pkg.variance_desc(), sparse=pkg.sparse_desc(block=B), holes=pkg.hole_desc(budget=budget))
    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    stream = torch.cuda.Stream(device=0)
    for r in range(frames):
        s.frame_device(walk[r % len(walk)], d_out.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    s.close()
    ctx.close()


def per_frame(path, frames, settle):
    """{kernel: (launches per frame, ms per frame)} over frames [settle, frames), and the GPU time from the first dispatch of a frame
    to the first of the next, averaged over them."""
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    frame, per, starts = -1, {}, []
    for r in rows:
        name = re.sub(r"\(.*", "", r["Kernel_Name"].replace("void ", "").replace("(anonymous namespace)::", ""))
        if name.startswith("k_sparse_rays"):
            frame += 1
            starts.append(int(r["Start_Timestamp"]))
        if settle <= frame < frames:
            c = per.setdefault(name, [0, 0.0])
            c[0] += 1
            c[1] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
    assert frame + 1 == frames, "%d frames in the trace, %d expected" % (frame + 1, frames)
    span = (starts[frames - 1] - starts[settle]) / 1e6 / (frames - 1 - settle)
    return {k: (c[0] / (frames - settle), c[1] / (frames - settle)) for k, c in per.items()}, span


def split(path, frames, settle, path0=None):
    a, span_a = per_frame(path, frames, settle)
    b, span_b = per_frame(path0, frames, settle) if path0 else ({}, 0.0)
    print("# frames %d .. %d of %d; launches and ms per frame: with hole rays%s" % (settle, frames - 1, frames, "; with budget 0" if path0 else ""))
    print("%-44s %9s %10s %9s %10s" % ("kernel", "launches", "ms", "launches", "ms"))
    for name in sorted(set(a) | set(b), key=lambda k: -(a.get(k, (0, 0))[1])):
        x, y = a.get(name, (0, 0.0)), b.get(name, (0, 0.0))
        print("%-44s %9.2f %10.4f %9.2f %10.4f" % (name[:44], x[0], x[1], y[0], y[1]))
    print("%-44s %9.2f %10.4f %9.2f %10.4f" % ("all kernels", sum(v[0] for v in a.values()), sum(v[1] for v in a.values()),
                                                 sum(v[0] for v in b.values()), sum(v[1] for v in b.values())))
    print("%-44s %9s %10.4f %9s %10.4f" % ("frame to frame, first dispatch to first", "", span_a, "", span_b))


if __name__ == "__main__":
    if len(sys.argv) == 5 and sys.argv[1] == "run":
        run(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]))
    elif len(sys.argv) in (5, 6) and sys.argv[1] == "split":
        split(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5] if len(sys.argv) == 6 else None)
    else:
        raise SystemExit(__doc__)
