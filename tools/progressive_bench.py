#!/usr/bin/env python3
"""Progressive rendering against the one-shot render (rtu_progressive_* vs rtu_render_frame_device /
rtu_render_frame_adaptive_device), one JSON line per workload, wall-clock milliseconds on the host (every progressive call is
synchronous; a one-shot frame is timed up to rtu_frame_status, which waits for the device), median of --runs after --warmup runs:
  first_snapshot_ms  session begin, advance(1), snapshot to the host: what a viewport waits for its first image
  doubling_ms        session begin, then passes of 1, 1, 2, 4, ... samples up to the target, a host snapshot after every pass
  doubling_device_ms the same with the snapshots left on the device (rtu_progressive_snapshot_device): the passes alone
  host_snapshot_ms   one host snapshot of a session (the float4 image copied to pageable host memory)
  one_shot_ms        the frame in one call, the image left on the device
and doubling / one-shot; then the drop-in (rtu_begin_render_progressive, one device, no PNG), which also creates a context, uploads
the scene and runs the host's gamma / Color24 post-pass into the RtuImage after every pass:
  dropin_first_pass_ms  from the begin call to the first on_pass
  dropin_ms             from the begin call to rtu_render_wait, doubling schedule
  dropin_one_shot_ms    the one-shot job of the same frame (rtu_begin_render_sampled / _paths / _adaptive): one post-pass

usage: tools/progressive_bench.py [--runs 5] [--warmup 2] [--out profiles/r06_progressive.json]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

# (name, golden tag of the scene, resolution (None: the tag's), samples, gather bounces, adaptive)
WORKLOADS = [("p11_1080 recipe P (config 5)", "p11_1080", None, 64, 4, False),
             ("teapot1_s2 recipe S 1920x1080", "teapot1_s2_160x90", (1920, 1080), 16, 0, False),
             ("p11_1080 recipe P adaptive, max 64", "p11_1080", None, 64, 4, True)]


def doubling(samples):
    out, done = [], 0
    while done < samples:
        k = min(max(done, 1), samples - done)
        out.append(k)
        done += k
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import __graft_entry__ as g
    pkg = g.load_package()
    ctx = pkg.Context(0)
    lines = []
    for name, tag, size, samples, gather, adaptive in WORKLOADS:
        scene = pkg.Scene.from_blob_file(os.path.join(REPO, "tests", "golden", tag, "scene.rtus.gz"))
        if size is None:
            meta = json.load(open(os.path.join(REPO, "tests", "golden", tag, "meta.json")))
            size = (meta["width"], meta["height"])
        W, H = size
        ctx.upload(scene)
        fr = pkg.frame_setup(scene.desc.camera, W, H, samples=samples, gather_bounces=gather)
        ad = pkg.adaptive_defaults() if adaptive else None
        d_rgbz = pkg.hip.rtu_device_alloc(ctx._h, W * H * 16)
        d_counts = pkg.hip.rtu_device_alloc(ctx._h, W * H)
        schedule = doubling(samples)

        def timed(run):
            for _ in range(args.warmup):
                run()
            ms = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                run()
                ms.append((time.perf_counter() - t0) * 1e3)
            return statistics.median(ms), ms

        def first_snapshot():
            s = ctx.progressive(fr, ad)
            s.advance(1)
            s.snapshot()
            s.close()

        def progressive():
            s = ctx.progressive(fr, ad)
            for n in schedule:
                s.advance(n)
                s.snapshot()
            s.close()

        def progressive_device():
            s = ctx.progressive(fr, ad)
            for n in schedule:
                s.advance(n)
                s.snapshot_device(d_rgbz, d_counts if samples <= 255 else None)
            ctx.frame_status()  # (waits for the device: the last snapshot)
            s.close()

        held = ctx.progressive(fr, ad)
        held.advance(1)

        def host_snapshot():
            held.snapshot()

        def one_shot():
            if adaptive:
                ctx._check(pkg.hip.rtu_render_frame_adaptive_device(ctx._h, ctypes.byref(fr), ctypes.byref(ad), d_rgbz, d_counts, None))
            else:
                ctx.render_device(fr, d_rgbz, None)
            ctx.frame_status()

        def dropin(progressive_job):
            img = pkg.Image(W, H)
            t = {}
            t0 = time.perf_counter()
            if progressive_job:
                job = pkg.ProgressiveJob(scene, img, [0], samples, gather, ad, None, lambda done, k: t.setdefault("first", time.perf_counter()))
                rc = job.wait()
                job.close()
            else:
                devs = (ctypes.c_int * 1)(0)
                if adaptive:
                    h = pkg.host.rtu_begin_render_adaptive(scene._h, img._h, devs, 1, samples, gather, ctypes.byref(ad), None, None, None)
                elif gather:
                    h = pkg.host.rtu_begin_render_paths(scene._h, img._h, devs, 1, samples, None, None)
                else:
                    h = pkg.host.rtu_begin_render_sampled(scene._h, img._h, devs, 1, samples, None, None)
                rc = pkg.host.rtu_render_wait(h)
                pkg.host.rtu_render_job_free(h)
            t1 = time.perf_counter()
            if rc != pkg.RTU_OK:
                raise SystemExit("%s: the job failed (%d): %s" % (name, rc, pkg.host.rtu_host_last_error().decode()))
            img.close()
            return (t1 - t0) * 1e3, (t.get("first", t1) - t0) * 1e3

        def timed_dropin(progressive_job):
            for _ in range(args.warmup):
                dropin(progressive_job)
            runs = [dropin(progressive_job) for _ in range(args.runs)]
            return [r[0] for r in runs], [r[1] for r in runs]

        first_ms, first_all = timed(first_snapshot)
        prog_ms, prog_all = timed(progressive)
        dev_ms, dev_all = timed(progressive_device)
        snap_ms, snap_all = timed(host_snapshot)
        held.close()
        one_ms, one_all = timed(one_shot)
        job_all, job_first_all = timed_dropin(True)
        job1_all, _ = timed_dropin(False)
        line = {"workload": name, "tag": tag, "width": W, "height": H, "samples": samples, "gather_bounces": gather, "adaptive": adaptive,
                "schedule": schedule, "first_snapshot_ms": round(first_ms, 3), "doubling_ms": round(prog_ms, 3), "one_shot_ms": round(one_ms, 3),
                "doubling_over_one_shot": round(prog_ms / one_ms, 4), "doubling_device_ms": round(dev_ms, 3),
                "doubling_device_over_one_shot": round(dev_ms / one_ms, 4), "host_snapshot_ms": round(snap_ms, 3),
                "dropin_first_pass_ms": round(statistics.median(job_first_all), 3), "dropin_ms": round(statistics.median(job_all), 3),
                "dropin_one_shot_ms": round(statistics.median(job1_all), 3),
                "runs_ms": {"first_snapshot": [round(x, 3) for x in first_all], "doubling": [round(x, 3) for x in prog_all],
                            "doubling_device": [round(x, 3) for x in dev_all], "host_snapshot": [round(x, 3) for x in snap_all],
                            "one_shot": [round(x, 3) for x in one_all], "dropin_first_pass": [round(x, 3) for x in job_first_all],
                            "dropin": [round(x, 3) for x in job_all], "dropin_one_shot": [round(x, 3) for x in job1_all]}}
        print(json.dumps(line), flush=True)
        lines.append(line)
        pkg.hip.rtu_device_free(ctx._h, d_rgbz)
        pkg.hip.rtu_device_free(ctx._h, d_counts)
    ctx.close()
    if args.out:
        with open(args.out, "w") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
