#!/usr/bin/env python3
"""What a temporally accumulated preview of a SENSOR costs (rtu_temporal_sensor_frame*, rtu_temporal_accumulate_sensor*), one JSON
line: Project11 as a 2048x1024 equirectangular recipe-P sensor of 16 samples inside the room, yawing one step per frame; a fisheye and
an orthographic sensor besides. Device figures are medians over `reps` regions bracketed by HIP events on one stream, after `warmup`
regions that are not counted; host figures are medians of the host clock around synchronous calls. Needs a GPU.

  session   a sensor frame of a plain session (with RTU_TEMPORAL_DENOISE) and of a variance session, per model, and for the panorama
            its parts as the session calls them, each bracketed on its own: rays (rtu_sensor_rays_device), shading
            (rtu_shade_rays_paths_device), centre rays, guides (rtu_ray_features_device), accumulation plain and moments
            (rtu_temporal_accumulate_sensor[_moments]_device), the filters.
  kernel    k_temporal_sensor<EQUIRECT, *> against k_temporal on buffers of the same size, alternating in the same run — each on the
            guides and the history of its own kind of frame —, and against a device copy of the bytes it must move: 80 B in, at
            least 48 B (moments 64 B) of taps, 64 B (80 B) out per pixel.
  follow    a session frame against the only way to follow a sensor without one, rtu_render_sensor with samples = 1 per pose;
            the two alternate in the same run, host clock, both synchronous.
  error     RMSE (linear rgb, all pixels) of the eighth frame of the yaw against rtu_render_sensor with 256 samples of that pose, as
            a fraction of the RMSE of that frame's raw sample: accumulated, accumulated and filtered, and the variance session.

usage: tools/sensor_temporal_bench.py [--reps 20] [--warmup 3] [--tag p11_1080] [--out profiles/r24_sensor_temporal.json]"""
import argparse
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

STEP_DEG = 0.25
S = 16


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tag", default="p11_1080")
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--height", type=int, default=1024)
    ap.add_argument("--reference-samples", type=int, default=256)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    import __graft_entry__ as g
    from conftest import Golden
    from test_gpu_sensor import scene_places
    from test_temporal_host import orbit_scene
    pkg = g.load_package()
    if not torch.cuda.is_available():
        raise SystemExit("sensor_temporal_bench: no GPU")
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    scene = Golden(args.tag).scene(pkg)
    W, H = args.width, args.height
    n = W * H
    ctx.upload(scene)
    places, (right, up, fwd), _ = scene_places(pkg, scene)
    right, up, fwd = (np.array(v, np.float64) for v in (right, up, fwd))
    dist = float(np.linalg.norm(np.array(places["camera"]) - np.array(places["inside"]))) / 0.8

    def sensor(model, k, samples=S, gather=4):
        a = math.radians(STEP_DEG * k)
        r2, f2 = right * math.cos(a) + fwd * math.sin(a), fwd * math.cos(a) - right * math.sin(a)
        pos = places["camera" if model == "ortho" else "inside"]
        return pkg.sensor_desc(model, W, H, pos, r2, up, f2, samples=samples, gather_bounces=gather, fov_deg=180.0, extent=(0.8 * dist, 0.8 * dist * H / W))
    steps = list(range(8)) + list(range(6, 0, -1))  # there and back: 14 steps
    poses = {m: [sensor(m, k) for k in steps] for m in ("equirect", "fisheye", "ortho")}
    cams = [pkg.frame_setup(orbit_scene(pkg, scene, k, 60.0, STEP_DEG).desc.camera, W, H, samples=S, gather_bounces=4) for k in steps]
    out = {"tool": "sensor_temporal_bench", "reps": args.reps, "warmup": args.warmup, "device": pkg.device_info(0)["name"], "scene": args.tag,
           "width": W, "height": H, "samples": S, "yaw_step_deg": STEP_DEG, "yaw_step_columns": STEP_DEG / 360.0 * W}
    turn = [0]

    def nxt(seq):
        turn[0] += 1
        return seq[turn[0] % len(seq)]

    def timed(launch, reps=args.reps):
        for _ in range(args.warmup):
            launch()
        stream.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            launch()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return summary(ms)

    d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    d_n = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()

    def open_session(kind):
        return ctx.temporal(pkg.temporal_desc(W, H, denoise=kind == "denoise"), variance=pkg.variance_desc(W, H) if kind == "variance" else None)

    # ---- session frames per model, and the panorama's parts ---------------------------------------------------------------------------
    ses = {}
    for model in ("equirect", "fisheye", "ortho"):
        for kind in ("plain", "denoise", "variance"):
            s = open_session(kind)
            r = timed(lambda: s.sensor_frame_device(nxt(poses[model]), d_out.data_ptr(), stream.cuda_stream))
            s.history_device(d_n.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            r["mean_history"] = float(d_n.mean().item())
            ses["%s_%s" % (model, kind)] = r
            s.close()
    z8 = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
    d_rays, d_keys, d_img, d_hits, d_alb, d_var = z8(32 * n), z8(4 * n), z8(16 * n), z8(48 * n), z8(16 * n), z8(4 * n)
    d_hist = [z8(64 * n) for _ in range(2)]
    c_hits, c_alb, c_hist = z8(48 * n), z8(16 * n), [z8(64 * n) for _ in range(2)]
    desc, vdesc, ddesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H), pkg.denoise_desc(W, H)
    eq = poses["equirect"]
    k = [0]
    P = lambda t: t.data_ptr()

    def rays():
        k[0] += 1
        ctx.sensor_rays_device(eq[k[0] % len(eq)], P(d_rays), P(d_keys), k[0] % S, 1, stream.cuda_stream)

    def shade():
        d = eq[k[0] % len(eq)]
        ctx.shade_rays_paths_device(P(d_rays), P(d_keys), n, tuple(d.pos), P(d_img), stream.cuda_stream, max_bounce=d.max_bounce)

    def centre():
        c = pkg.RtuSensorDesc.from_buffer_copy(bytes(eq[k[0] % len(eq)]))
        c.samples, c.gather_bounces = 0, 0
        ctx.sensor_rays_device(c, P(d_rays), None, 0, 1, stream.cuda_stream)

    def accumulate_sensor(moments):
        def run():
            k[0] += 1
            a, b = d_hist[k[0] & 1], d_hist[(k[0] + 1) & 1]
            ctx.temporal_accumulate_sensor_device(desc, eq[(k[0] - 1) % len(eq)], eq[k[0] % len(eq)], P(d_img), P(d_hits), P(d_alb), P(a), P(b), P(d_out),
                                                  moments=moments, stream=stream.cuda_stream)
        return run

    def accumulate_camera():
        k[0] += 1
        a, b = c_hist[k[0] & 1], c_hist[(k[0] + 1) & 1]
        ctx.temporal_accumulate_device(desc, cams[(k[0] - 1) % len(cams)], cams[k[0] % len(cams)], P(d_img), P(c_hits), P(c_alb), P(a), P(b), P(d_out),
                                       stream.cuda_stream)
    parts = {"rays": timed(rays)}
    parts["shading"] = timed(shade)
    try:
        ctx.frame_status()
        parts["shading_complete"] = True
    except pkg.RtuError:  # (the sessions above have grown the frame records: not expected)
        parts["shading_complete"] = False
    parts["centre_rays"] = timed(centre)
    parts["guides"] = timed(lambda: ctx.ray_features_device(P(d_rays), n, P(d_hits), P(d_alb), stream.cuda_stream))
    ctx.frame_features_device(cams[0], P(c_hits), P(c_alb), stream.cuda_stream)
    # histories to look up: one frame without a previous one, of each form and kind
    ctx.temporal_accumulate_sensor_device(desc, None, eq[0], P(d_img), P(d_hits), P(d_alb), None, P(d_hist[0]), P(d_out), moments=True, stream=stream.cuda_stream)
    ctx.temporal_accumulate_sensor_device(desc, None, eq[0], P(d_img), P(d_hits), P(d_alb), None, P(d_hist[1]), P(d_out), moments=True, stream=stream.cuda_stream)
    ctx.temporal_accumulate_device(desc, None, cams[0], P(d_img), P(c_hits), P(c_alb), None, P(c_hist[0]), P(d_out), stream.cuda_stream)
    ctx.temporal_accumulate_device(desc, None, cams[0], P(d_img), P(c_hits), P(c_alb), None, P(c_hist[1]), P(d_out), stream.cuda_stream)
    stream.synchronize()
    # the kernels alternate: sensor plain, camera, sensor moments, and again
    rounds = {"k_temporal_sensor_equirect_plain": [], "k_temporal": [], "k_temporal_sensor_equirect_moments": []}
    runs = {"k_temporal_sensor_equirect_plain": accumulate_sensor(False), "k_temporal": accumulate_camera, "k_temporal_sensor_equirect_moments": accumulate_sensor(True)}
    for r in range(3):
        for name, run in runs.items():
            rounds[name].append(timed(run, max(5, args.reps // 2))["median_ms"])
    kern = {name: {"median_ms": statistics.median(v), "rounds_ms": v} for name, v in rounds.items()}
    parts["accumulation"] = kern["k_temporal_sensor_equirect_plain"]
    parts["accumulation_moments"] = kern["k_temporal_sensor_equirect_moments"]
    parts["filter_denoise"] = timed(lambda: ctx.denoise_device(ddesc, P(d_out), P(d_hits), P(d_alb), P(d_out), stream.cuda_stream))

    def variance_filter():
        ctx.variance_device(vdesc, P(d_hist[0]), P(d_hits), P(d_var), stream.cuda_stream)
        ctx.denoise_variance_device(vdesc, P(d_out), P(d_hits), P(d_alb), P(d_var), P(d_out), stream.cuda_stream)
    parts["filter_variance"] = timed(variance_filter)
    parts["sum_plain_denoise_ms"] = sum(parts[p]["median_ms"] for p in ("rays", "shading", "centre_rays", "guides", "accumulation", "filter_denoise"))
    parts["sum_variance_ms"] = sum(parts[p]["median_ms"] for p in ("rays", "shading", "centre_rays", "guides", "accumulation_moments", "filter_variance"))
    ses["equirect_parts"] = parts
    out["session"] = ses

    # ---- the kernel against k_temporal and against a copy of its bytes ----------------------------------------------------------------
    src, dst = z8(n * 144), z8(n * 144)
    with torch.cuda.stream(stream):
        copies = {b: timed(lambda b=b: dst[:n * b].copy_(src[:n * b])) for b in (64, 80, 128, 144)}
    # a copy of B bytes reads B and writes B: 128 B read + 64 B written is (copy of 128 + copy of 64) / 2; moments: 144 B and 80 B
    floor = 0.5 * (copies[128]["median_ms"] + copies[64]["median_ms"])
    floor_m = 0.5 * (copies[144]["median_ms"] + copies[80]["median_ms"])
    kern.update({"copy_ms": {str(b): c for b, c in copies.items()}, "floor_plain_ms": floor, "floor_moments_ms": floor_m,
                 "sensor_plain_over_k_temporal": kern["k_temporal_sensor_equirect_plain"]["median_ms"] / kern["k_temporal"]["median_ms"],
                 "sensor_plain_over_floor": kern["k_temporal_sensor_equirect_plain"]["median_ms"] / floor,
                 "sensor_moments_over_floor": kern["k_temporal_sensor_equirect_moments"]["median_ms"] / floor_m,
                 "k_temporal_over_floor": kern["k_temporal"]["median_ms"] / floor})
    out["kernel"] = kern

    # ---- following a sensor: a session frame against rtu_render_sensor with one sample per pose, alternating ----------------------------
    s = open_session("denoise")
    a_ms, b_ms = [], []
    for r in range(args.warmup + args.reps):
        d = nxt(eq)
        one = pkg.RtuSensorDesc.from_buffer_copy(bytes(d))
        one.samples = 1
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        s.sensor_frame_device(d, P(d_out), stream.cuda_stream)
        stream.synchronize()
        t1 = time.perf_counter()
        ctx.render_sensor_device(one, P(d_out), stream.cuda_stream)
        stream.synchronize()
        t2 = time.perf_counter()
        a_ms.append((t1 - t0) * 1e3)
        b_ms.append((t2 - t1) * 1e3)
    s.close()
    out["follow"] = {"session_frame_host_ms": summary(a_ms[args.warmup:]), "render_sensor_1spp_host_ms": summary(b_ms[args.warmup:]),
                     "session_over_render": statistics.median(a_ms[args.warmup:]) / statistics.median(b_ms[args.warmup:])}

    # ---- the error of the eighth frame of the yaw ---------------------------------------------------------------------------------
    last = eq[7]
    ref_desc = pkg.RtuSensorDesc.from_buffer_copy(bytes(last))
    ref_desc.samples = args.reference_samples
    ref = ctx.render_sensor(ref_desc)[..., :3].astype(np.float64)

    def rmse(img):
        return float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref) ** 2)))
    ctx.sensor_rays_device(last, P(d_rays), P(d_keys), 7 % S, 1, stream.cuda_stream)
    ctx.shade_rays_paths_device(P(d_rays), P(d_keys), n, tuple(last.pos), P(d_img), stream.cuda_stream, max_bounce=last.max_bounce)
    ctx.frame_status()
    raw = rmse(d_img.cpu().numpy().view(np.float32).reshape(H, W, 4))
    err = {"reference_samples": args.reference_samples, "raw_sample_rmse": raw}
    for kind in ("plain", "denoise", "variance"):
        s = open_session(kind)
        for j in range(8):
            img = s.sensor_frame(eq[j])
        err["%s_over_raw" % kind] = rmse(img) / raw
        err["%s_mean_history" % kind] = float(s.history().mean())
        s.close()
    out["error"] = err
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
