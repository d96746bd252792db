"""GPU: temporal gradients (include/rtu_render.h "Temporal gradients"). The four device forms (rtu_gradient_rays_device,
rtu_sample_luminance_device, rtu_temporal_gradient_device, rtu_temporal_accumulate_gradient_device) against their host forms (which
tests/test_gradient_host.py holds to the rules), bit for bit; a gradient session's frames, plain and moved, on a variance and on a
steered base, against the same steps assembled by hand; the exact zero of a scene at rest; a light that moves between two frames; the
session's contract."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES
from test_gpu_ray_query import bits
from test_gpu_temporal import dev, orbit_frames
from test_gpu_temporal_motion import animated
from test_gpu_variance import ctx, fresh, same_bytes  # noqa: F401 (ctx: a fixture)
from test_gradient_host import gradient_samples, np_owners, random_lambda, relit, strata
from test_steer_host import lens_camera
from test_temporal_host import FRAMES, chain_inputs
from test_temporal_motion_host import CASES, case_cameras, table
from test_variance_host import all_chains, moments_chain

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32


def back(d, dtype, shape):
    return d.cpu().numpy().view(dtype).reshape(shape)


# ---- 1. the device forms against the host forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_gradient_rays_device_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    sw, sh = strata(W, H)
    m, pad = sw * sh, 3
    stream = torch.cuda.Stream(device=0)
    for i, (S, sample, k) in enumerate(((1, 0, 0), (16, 15, 1), (4, 2, 0xffffffff), (16, 0, 9))):
        frame = lens_camera(pkg, W, H, S)
        gd = pkg.gradient_desc(W, H, frame_index=k)
        rays, keys, owner = pkg.gradient_rays(frame, sample, gd)
        d_rays, d_keys, d_owner = fresh(32 * (m + pad)), fresh(4 * (m + pad)), fresh(4 * (m + pad))
        s = stream if i % 2 else None
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.gradient_rays_device(gd, frame, sample, d_rays.data_ptr(), d_keys.data_ptr(), d_owner.data_ptr(), s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        for what, d, w, size_of in (("rays", d_rays, rays, 32), ("keys", d_keys, keys, 4), ("owner", d_owner, owner, 4)):
            got = d.cpu().numpy()
            assert got[:size_of * m].tobytes() == w.tobytes(), "%s differ (%s)" % (what, (S, sample, k))
            assert (got[size_of * m:] == 0x5A).all(), "%s: written beyond the strata" % what


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_gradient_device_equals_the_host_form(pkg, ctx, size):
    """The luminance plane, the gradients and lambda over section 24's twelve chains, with the NaN / infinite / zero samples, the taps
    outside the image and the rejected taps of tests/test_gradient_host.py."""
    import torch
    W, H = size
    sw, sh = strata(W, H)
    m = sw * sh
    stream = torch.cuda.Stream(device=0)
    taken = 0
    for ci, (kind, n, camname, cap, over) in enumerate(CASES):
        cams = case_cameras(pkg, W, H, camname)
        frames = chain_inputs(pkg, W, H, 1234 + ci)
        desc = pkg.temporal_desc(W, H, **over)
        motion = table(kind)[:n]
        res = moments_chain(pkg, cams, frames, desc, motion, cap)
        d_motion = dev(motion) if len(motion) else fresh(96)
        gsize = pkg.gradient_desc(W, H)
        for k in range(FRAMES):
            rgbz, hits, albedo = frames[k]
            d_rgbz, d_hits, d_alb = dev(rgbz), dev(hits), dev(albedo)
            d_lum = fresh(4 * W * H)
            ctx.sample_luminance_device(gsize, d_rgbz.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_lum.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(bits(back(d_lum, F, (H, W))), bits(pkg.sample_luminance(rgbz, hits, albedo))), "the luminance plane, frame %d" % k
            x, y = np_owners(W, H, k)
            owner = (x + W * y).astype(U)
            rgbt = gradient_samples(frames, k, owner, 100 * ci + k) if k else np.ones((m, 4), F)
            hist_prev = np.ascontiguousarray(res[k - 1][1]) if k else None
            lum_prev = pkg.sample_luminance(*frames[k - 1]) if k else None
            d_hist, d_lp = (dev(hist_prev), dev(lum_prev)) if k else (None, None)
            d_owner, d_rgbt = dev(owner), dev(rgbt)
            for j, (radius, kappa) in enumerate(((0, 0.0), (1, 2.0), (3, 2.0))):
                gd = pkg.gradient_desc(W, H, radius=radius, kappa=kappa)
                wd, wl = pkg.temporal_gradient(cams[k - 1] if k else None, cams[k], hits, albedo, motion, hist_prev, lum_prev, owner, rgbt, desc, gd)
                d_diff, d_lam = fresh(16 * m + 16), fresh(4 * m + 4)
                s = stream if (k + j) % 2 else None
                torch.cuda.synchronize()
                a0 = pkg.hip.rtu_debug_device_allocations()
                ctx.temporal_gradient_device(desc, gd, cams[k - 1] if k else None, cams[k], d_hits.data_ptr(), d_alb.data_ptr(), d_motion.data_ptr(), len(motion),
                                             d_hist.data_ptr() if k else None, d_lp.data_ptr() if k else None, d_owner.data_ptr(), d_rgbt.data_ptr(),
                                             d_diff.data_ptr(), d_lam.data_ptr(), s.cuda_stream if s else None)
                (s or torch.cuda).synchronize()
                assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
                what = "table %s[%d] cameras %s frame %d radius %d kappa %g" % (kind, n, camname, k, radius, kappa)
                gdiff, glam = d_diff.cpu().numpy(), d_lam.cpu().numpy()
                assert (gdiff[16 * m:] == 0x5A).all() and (glam[4 * m:] == 0x5A).all(), what + ": written beyond the strata"
                for name, g, w in (("diff", gdiff[:16 * m].view(F).reshape(sh, sw, 4), wd), ("lambda", glam[:4 * m].view(F).reshape(sh, sw), wl)):
                    bad = bits(g) != bits(w)
                    assert not bad.any(), "%s %s: %d words differ, first at %s" % (what, name, bad.sum(), np.argwhere(bad)[0])
                taken += int((wl > 0).sum())
            assert same_bytes(d_hits, hits) and same_bytes(d_alb, albedo) and same_bytes(d_owner, owner) and same_bytes(d_rgbt, rgbt), "an input was written"
            assert not k or (same_bytes(d_hist, hist_prev) and same_bytes(d_lp, lum_prev)), "an input was written"
    assert taken > 0 or size == (1, 1)


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_capped_accumulator_device_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    streams = (None, torch.cuda.Stream(device=0))
    changed = 0
    for ci, (what, cams, frames, desc, motion, cap) in enumerate(all_chains(pkg, W, H)):
        d_motion = dev(motion) if len(motion) else fresh(96)
        hist = None
        plain = moments_chain(pkg, cams, frames, desc, motion, cap)
        for k in range(FRAMES):
            rgbz, hits, albedo = frames[k]
            lam = random_lambda(W, H, 31 * ci + k)
            prev = cams[k - 1] if k else None
            want = pkg.temporal_accumulate_gradient(prev, cams[k], rgbz, hits, albedo, motion, hist, desc, cap, lam)
            d_in, d_hits, d_alb, d_lam = dev(rgbz), dev(hits), dev(albedo), dev(lam)
            d_prev = dev(hist) if hist is not None else None
            d_hist = fresh(4 * H * W * 16)
            in_place = k == 2  # rgbz_out == rgbz is allowed
            d_out = d_in if in_place else fresh(H * W * 16)
            s = streams[k % 2]
            torch.cuda.synchronize()
            a0 = pkg.hip.rtu_debug_device_allocations()
            ctx.temporal_accumulate_gradient_device(desc, prev, cams[k], d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                                    d_prev.data_ptr() if d_prev is not None else None, d_hist.data_ptr(), d_out.data_ptr(), d_motion.data_ptr(),
                                                    len(motion), cap, d_lam.data_ptr(), s.cuda_stream if s else None)
            (s or torch.cuda).synchronize()
            assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
            for name, g, w in (("image", back(d_out, F, (H, W, 4)), want[0]), ("history", back(d_hist, F, (4, H, W, 4)), want[1])):
                bad = bits(g) != bits(w)
                assert not bad.any(), "%s frame %d %s: %d words differ, first at %s" % (what, k, name, bad.sum(), np.argwhere(bad)[0])
            assert same_bytes(d_lam, lam) and same_bytes(d_hits, hits) and (in_place or same_bytes(d_in, rgbz)), "an input was written"
            if k == 3:  # no lambda: the moments form
                d_h2, d_o2 = fresh(4 * H * W * 16), fresh(H * W * 16)
                d_p2 = dev(plain[k - 1][1])
                ctx.temporal_accumulate_gradient_device(desc, prev, cams[k], d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_p2.data_ptr(), d_h2.data_ptr(),
                                                        d_o2.data_ptr(), d_motion.data_ptr(), len(motion), cap, None)
                torch.cuda.synchronize()
                assert np.array_equal(bits(back(d_h2, F, (4, H, W, 4))), bits(plain[k][1])) and np.array_equal(bits(back(d_o2, F, (H, W, 4))), bits(plain[k][0]))
            changed += int((bits(want[1]) != bits(plain[k][1])).sum())
            hist = want[1]
    assert changed > 0


def test_device_refusals(pkg, ctx):
    import torch
    W, H = 7, 5
    n, m = W * H, 6
    buf = torch.zeros(4096 + 400 * n, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 16 == 0
    d_hits, d_alb, d_motion, d_hist, d_lum, d_owner, d_rgbt, d_diff, d_lam = (base + 16 * i for i in (0, 3 * n, 4 * n, 4 * n + 18, 8 * n + 18, 9 * n + 18, 10 * n + 18, 11 * n + 18, 12 * n + 18))
    d_rgbz, d_hout, d_rays, d_keys = (base + 16 * i for i in (13 * n + 18, 14 * n + 18, 18 * n + 18, 20 * n + 18))
    prev, cur = lens_camera(pkg, W, H, 4), lens_camera(pkg, W, H, 4)
    td, gd = pkg.temporal_desc(W, H), pkg.gradient_desc(W, H)
    ref = lambda d: ctypes.byref(d) if d is not None else None

    def grad(t=td, g=gd, p=prev, c=cur, a=None):
        a = a or [d_hits, d_alb, d_motion, 3, d_hist, d_lum, d_owner, d_rgbt, d_diff, d_lam]
        return pkg.hip.rtu_temporal_gradient_device(ctx._h, ref(t), ref(g), ref(p), ref(c), *a, None)

    def rays(g=gd, f=cur, sample=1, a=None):
        return pkg.hip.rtu_gradient_rays_device(ctx._h, ref(g), ref(f), sample, *(a or [d_rays, d_keys, d_owner]), None)

    def lum(g=gd, a=None):
        return pkg.hip.rtu_sample_luminance_device(ctx._h, ref(g), *(a or [d_rgbz, d_hits, d_alb, d_lum]), None)

    def acc(t=td, p=prev, a=None, c=0):
        a = a or [d_rgbz, d_hits, d_alb, d_hist, d_hout, d_rgbz, d_motion]
        return pkg.hip.rtu_temporal_accumulate_gradient_device(ctx._h, ref(t), ref(p), ref(cur), a[0], a[1], a[2], a[3], a[4], a[5], a[6], 3, c, d_lam, None)

    assert grad() == rays() == lum() == acc() == pkg.RTU_OK
    full = [d_hits, d_alb, d_motion, 3, d_hist, d_lum, d_owner, d_rgbt, d_diff, d_lam]
    for i in (0, 1, 2, 5, 6, 7, 8, 9):
        assert grad(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    for i in (0, 1, 2, 4, 5, 6, 7, 8, 9):
        assert grad(a=[p + 2 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    for i in (0, 1, 2, 4, 7, 8):  # float4 buffers: 16-byte aligned
        assert grad(a=[p + 4 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    assert grad(p=None) == pkg.RTU_ERR_ARG and grad(p=None, a=full[:4] + [None, None] + full[6:]) == pkg.RTU_OK
    assert grad(t=None) == grad(g=None) == grad(c=None) == grad(g=pkg.gradient_desc(W + 1, H)) == grad(p=lens_camera(pkg, W, H + 1, 4)) == pkg.RTU_ERR_ARG
    for bad in ({"radius": -1}, {"radius": 4}, {"kappa": -1.0}, {"kappa": float("nan")}, {"enabled": 2}, {"width": 0}):
        g = pkg.gradient_desc(W, H)
        for key, v in bad.items():
            setattr(g, key, v)
        assert grad(g=g) == rays(g=g) == lum(g=g) == pkg.RTU_ERR_ARG, bad
    g = pkg.gradient_desc(W, H)
    g.reserved[1] = 1
    assert grad(g=g) == rays(g=g) == lum(g=g) == pkg.RTU_ERR_ARG
    for i in range(3):
        full = [d_rays, d_keys, d_owner]
        assert rays(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
        assert rays(a=[p + 2 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    assert rays(a=[d_rays + 8, d_keys, d_owner]) == rays(sample=4) == rays(sample=-1) == rays(f=None) == rays(f=lens_camera(pkg, W + 1, H, 4)) == pkg.RTU_ERR_ARG
    for i in range(4):
        full = [d_rgbz, d_hits, d_alb, d_lum]
        assert lum(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
        assert lum(a=[p + 2 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    full = [d_rgbz, d_hits, d_alb, d_hist, d_hout, d_rgbz, d_motion]
    for i in (0, 1, 2, 4, 5, 6):
        assert acc(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    for i in range(7):
        assert acc(a=[p + 4 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    assert acc(a=full[:4] + [d_hist + 16] + full[5:]) == pkg.RTU_ERR_ARG, "overlapping histories"
    assert acc(c=-1) == acc(c=65536) == acc(t=None) == acc(p=None) == acc(t=pkg.temporal_desc(W, H, max_history=0)) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_temporal_accumulate_gradient_device(ctx._h, ref(td), ref(prev), ref(cur), d_rgbz, d_hits, d_alb, d_hist, d_hout, d_rgbz, d_motion, 3, 0,
                                                           d_lam + 2, None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_gradient_rays_device(None, ref(gd), ref(cur), 1, d_rays, d_keys, d_owner, None) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()


# ---- 2. sessions against the hand-assembled form ------------------------------------------------------------------------------------
def hand_frame(pkg, ctx, frame, k, prev, state, desc, vdesc, sdesc, gdesc, motion, cap, steer_out=None):
    """Frame k by hand. The rays of the frame and, with a previous frame, the gradient rays of rtu_gradient_rays_device behind them in
    ONE batch through the existing ray-batch shading; frame_features; rtu_temporal_gradient_device, rtu_temporal_accumulate_gradient_device
    and rtu_sample_luminance_device; then the variance session's (and the steered session's) steps by their host forms.
    state: (history, luminance plane) of the frame before, or None. steer_out: a dict that takes the steered steps' counts and total."""
    import torch
    W, H = frame.width, frame.height
    n = W * H
    sw, sh = strata(W, H)
    m = sw * sh
    rays, keys = pkg.camera_sample_rays(frame, k % frame.samples)
    d_owner = None
    if state is not None:
        gd = pkg.gradient_desc(W, H, radius=gdesc.radius, kappa=gdesc.kappa, frame_index=k)
        d_gr, d_gk, d_owner = fresh(32 * m), fresh(4 * m), fresh(4 * m)
        ctx.gradient_rays_device(gd, frame, (k - 1) % frame.samples, d_gr.data_ptr(), d_gk.data_ptr(), d_owner.data_ptr())
        torch.cuda.synchronize()
        rays = np.concatenate([rays, d_gr.cpu().numpy().view(pkg.ray_dtype())])
        keys = np.concatenate([keys, d_gk.cpu().numpy().view(U)])
    shade = ctx.shade_rays_paths if frame.gather_bounces else ctx.shade_rays_sampled
    rgbt = shade(rays, keys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0]
    sample = np.ascontiguousarray(rgbt[:n]).reshape(H, W, 4)
    hits, albedo = ctx.frame_features(frame)
    d_in, d_hits, d_alb, d_motion = dev(sample), dev(hits), dev(albedo), dev(motion)
    d_hist, d_out, d_lum, d_lam = fresh(64 * n), fresh(16 * n), fresh(4 * n), None
    lam = np.zeros((sh, sw), F)
    if state is not None:
        d_prev, d_lp, d_rgbt = dev(state[0]), dev(state[1]), dev(np.ascontiguousarray(rgbt[n:]))
        d_diff, d_lam = fresh(16 * m), fresh(4 * m)
        ctx.temporal_gradient_device(desc, gd, prev, frame, d_hits.data_ptr(), d_alb.data_ptr(), d_motion.data_ptr(), len(motion), d_prev.data_ptr(),
                                     d_lp.data_ptr(), d_owner.data_ptr(), d_rgbt.data_ptr(), d_diff.data_ptr(), d_lam.data_ptr())
        ctx.temporal_accumulate_gradient_device(desc, prev, frame, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_prev.data_ptr(), d_hist.data_ptr(),
                                                d_out.data_ptr(), d_motion.data_ptr(), len(motion), cap, d_lam.data_ptr())
    else:
        ctx.temporal_accumulate_gradient_device(desc, None, frame, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), None, d_hist.data_ptr(), d_out.data_ptr(),
                                                d_motion.data_ptr(), len(motion), cap, None)
    ctx.sample_luminance_device(pkg.gradient_desc(W, H), d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_lum.data_ptr())
    torch.cuda.synchronize()
    out, hist, lum = back(d_out, F, (H, W, 4)).copy(), back(d_hist, F, (4, H, W, 4)).copy(), back(d_lum, F, (H, W)).copy()
    if d_lam is not None:
        lam = back(d_lam, F, (sh, sw)).copy()
    v = pkg.variance(hist, hits, vdesc)
    if sdesc is not None:
        sd = pkg.steer_desc(W, H, budget=sdesc.budget, max_extra=sdesc.max_extra, frame_index=k)
        counts, offsets, total = pkg.sample_allocation(hist, hits, v, sd)
        if steer_out is not None:
            steer_out.update(counts=counts, total=total)
        if total:
            xrays, xkeys, _ = pkg.extra_sample_rays(frame, counts, offsets, sd)
            xrgbt = shade(xrays, xkeys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0]
            out, hist = pkg.temporal_refine(hist, out, hits, albedo, counts, offsets, xrgbt, desc)
            v = pkg.variance(hist, hits, vdesc)
    yg, xg = np.mgrid[0:H, 0:W]
    return pkg.denoise_variance(out, hits, albedo, v, vdesc), (hist, lum), lam[yg // 3, xg // 3]


@pytest.mark.parametrize("tag,kw,distance", [("p10_s4_160x120", {"samples": 3}, 20.0), ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0)],
                         ids=["S", "P"])
@pytest.mark.parametrize("steered", [False, True], ids=["variance", "steered"])
def test_session_equals_the_hand_form(pkg, ctx, golden, tag, kw, distance, steered):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    frames = orbit_frames(pkg, scene, W, H, 3, distance, 0.5, **kw)
    frames = [frames[0], frames[0], frames[1], frames[2]]  # a frame at rest (the one-tap path), then a moving camera
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    sdesc = pkg.steer_desc(budget=W * H // 2, max_extra=3) if steered else None
    gdesc = pkg.gradient_desc(radius=1, kappa=0.5)  # a low noise floor: lambda is above 0 under the moving camera
    still = table("static", scene.desc.n_nodes)
    s = ctx.temporal(desc, variance=pkg.variance_desc(), steer=sdesc, gradient=gdesc)
    try:
        assert not s.lambda_image().any()
        prev = state = None
        taken = 0
        for k, frame in enumerate(frames):
            got = s.frame(frame)
            want, state, lam = hand_frame(pkg, ctx, frame, k, prev, state, desc, vdesc, sdesc, gdesc, still, 0)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(state[0][0][..., 3]))
            assert np.array_equal(bits(s.lambda_image()), bits(lam)), "frame %d: lambda" % k
            assert k != 1 or not lam.any(), "camera at rest, nothing changed: lambda is 0"
            taken += int((lam > 0).sum())
        assert taken > 0, "no gradient under the moving camera"
    finally:
        s.close()


@pytest.mark.parametrize("steered", [False, True], ids=["variance", "steered"])
def test_moved_session_equals_the_hand_form(pkg, ctx, golden, steered):
    g = golden("p10_s4_160x120")
    W, H = g.width, g.height
    scenes = animated(pkg, g.scene(pkg), 3, 20.0, 0.2)
    frames = [pkg.frame_setup(sc.desc.camera, W, H, samples=3) for sc in scenes]
    ctx.upload(scenes[0])
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    sdesc = pkg.steer_desc(budget=W * H, max_extra=2) if steered else None
    gdesc = pkg.gradient_desc(radius=2, kappa=1.0)
    s = ctx.temporal(desc, variance=vdesc, steer=sdesc, gradient=gdesc)
    try:
        prev = state = None
        taken = 0
        for k, frame in enumerate(frames):
            if k:
                ctx.update(scenes[k])  # rtu_update_scene
            motion = pkg.scene_motion(scenes[k - 1] if k else scenes[0], scenes[k])
            want, state, lam = hand_frame(pkg, ctx, frame, k, prev, state, desc, vdesc, sdesc, gdesc, motion, 3)
            got = s.frame_moved(frame, motion, 3)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(state[0][0][..., 3])) and np.array_equal(bits(s.lambda_image()), bits(lam))
            taken += int((lam > 0).sum())
        assert taken > 0, "no gradient although nodes moved"
    finally:
        s.close()


# ---- 3. a scene at rest, and a light that moves -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag,kw", [("p11gs_s2_160x90", {"samples": 16}), ("p11_p2_120x68", {"samples": 16, "gather_bounces": 4})], ids=["S", "P"])
def test_a_scene_at_rest_is_a_variance_session(pkg, ctx, golden, tag, kw):
    """Camera at rest, nothing changed: the gradient ray is the previous frame's ray with the previous frame's key, shaded at another
    position of a larger batch — lambda is 0.0 everywhere and the images are a variance session's bit for bit."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    frame = pkg.frame_setup(scene.desc.camera, W, H, **kw)
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc()
    a, b = ctx.temporal(desc, variance=vdesc, gradient=pkg.gradient_desc()), ctx.temporal(desc, variance=vdesc)
    try:
        for k in range(4):
            got, want = a.frame(frame), b.frame(frame)
            lam = a.lambda_image()
            assert not bits(lam).any(), "frame %d: lambda != 0.0 in %d pixels, max %g" % (k, (bits(lam) != 0).sum(), lam.max())
            assert np.array_equal(bits(got), bits(want)), "frame %d: not the variance session's image" % k
            assert np.array_equal(bits(a.history()), bits(b.history()))
    finally:
        a.close()
        b.close()


def test_a_light_moved_between_two_frames(pkg, orc, ctx, golden):
    g = golden("p11gs_s2_160x90")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    after = relit(pkg, scene, "moved")
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=16)
    motion = pkg.scene_motion(scene, after)
    assert (motion["flags"] == 1).all(), "every node is RTU_MOTION_STATIC"
    ctx.upload(scene)
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc()
    a, b = ctx.temporal(desc, variance=vdesc, gradient=pkg.gradient_desc()), ctx.temporal(desc, variance=vdesc)
    try:
        for k in range(6):
            a.frame(frame)
            b.frame(frame)
        assert not a.lambda_image().any()
        ctx.update(after)
        got, plain = a.frame_moved(frame, motion), b.frame_moved(frame, motion)
        lam, ha, hb = a.lambda_image(), a.history(), b.history()
        sw, sh = strata(W, H)
        lam_s = lam[::3, ::3]
        assert lam_s.shape == (sh, sw)
        share = float((lam_s > 0).mean())
        print("lambda > 0 in %.1f %% of the strata, mean %.3f; mean history %.2f against %.2f" % (100 * share, lam_s.mean(), ha.mean(), hb.mean()))
        assert share > 0.30, "lambda > 0 in %.1f %% of the strata" % (100 * share)
        assert (hb == 7).mean() > 0.9, "the variance session kept its history"
        hit = lam > 0
        assert (ha[hit] <= hb[hit]).all() and ha[hit].mean() < hb[hit].mean()
        with np.errstate(divide="ignore"):
            binding = hit & (F(1.0) / lam - F(1.0) < hb - 1)  # the cap is below what the variance session took over
        assert binding.any() and (ha[binding] < hb[binding]).all(), "a capped pixel kept its history"
        ref = orc.render_samples(after, W, H, 256, threads=8)[0]
        err = lambda img: float(np.sqrt(np.mean((img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2)))
        print("RMSE against 256 spp: gradient session %.5f, variance session %.5f" % (err(got), err(plain)))
        assert err(got) < err(plain)
    finally:
        a.close()
        b.close()


# ---- 4. the contract ---------------------------------------------------------------------------------------------------------------
def test_session_contract(pkg, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    frames = orbit_frames(pkg, scene, W, H, 4, 20.0, 0.5, samples=4)
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc()
    sdesc = pkg.steer_desc(budget=W * H // 4, max_extra=3)
    c = pkg.Context(0)
    try:
        a = c.temporal(desc, variance=vdesc, gradient=pkg.gradient_desc(kappa=0.5))
        with pytest.raises(pkg.RtuError) as e:      # before an upload
            a.frame(frames[0])
        assert e.value.code == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        # enabled == 0: the parent session's bits, on a variance and on a steered base
        for steer in (None, sdesc):
            off = c.temporal(desc, variance=vdesc, steer=steer, gradient=pkg.gradient_desc(enabled=0))
            parent = c.temporal(desc, variance=vdesc, steer=steer)
            for f in frames[:3]:
                assert np.array_equal(bits(off.frame(f)), bits(parent.frame(f))) and not off.lambda_image().any()
            off.close()
            parent.close()
        plain = c.temporal(desc, variance=vdesc)
        assert not plain.lambda_image().any(), "no gradient session: zeros"
        differs = 0
        for k, f in enumerate(frames):
            a0 = pkg.hip.rtu_debug_device_allocations()
            got = a.frame(f)
            assert k == 0 or pkg.hip.rtu_debug_device_allocations() == a0, "frame %d of a gradient session allocated" % k
            differs += int((bits(got) != bits(plain.frame(f))).sum())
            assert k > 0 or not a.lambda_image().any(), "frame 0 takes no gradient"
        assert differs > 0 and a.lambda_image().any(), "the gradients changed nothing under a moving camera"
        # reset, and a plain frame after an update, start over
        a.reset()
        assert not a.lambda_image().any() and not a.history().any()
        a.frame(frames[0])
        assert not a.lambda_image().any() and a.history().max() == 1
        a.frame(frames[1])
        assert a.history().max() == 2
        c.update(scene)
        a.frame(frames[2])
        assert not a.lambda_image().any() and a.history().max() == 1, "a plain frame after an update starts over"
        # the refusals
        for over in ({"radius": -1}, {"radius": 4}, {"kappa": -1.0}, {"kappa": float("nan")}, {"enabled": 2}):
            with pytest.raises(pkg.RtuError) as e:
                c.temporal(desc, variance=vdesc, gradient=pkg.gradient_desc(**over))
            assert e.value.code == pkg.RTU_ERR_ARG, over
        bd = pkg.gradient_desc()
        bd.reserved[0] = 1
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=vdesc, gradient=bd)
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=pkg.variance_desc(n_passes=0), gradient=pkg.gradient_desc())
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=vdesc, steer=pkg.steer_desc(max_extra=0), gradient=pkg.gradient_desc())
        err, gd = ctypes.c_int(0), pkg.gradient_desc()
        begin = pkg.hip.rtu_temporal_begin_gradient
        assert not begin(None, ctypes.byref(desc), ctypes.byref(vdesc), None, ctypes.byref(gd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not begin(c._h, ctypes.byref(desc), ctypes.byref(vdesc), None, None, ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not begin(c._h, ctypes.byref(desc), None, None, ctypes.byref(gd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not begin(c._h, None, ctypes.byref(vdesc), None, ctypes.byref(gd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_lambda_device(a._h, None, None) == pkg.RTU_ERR_ARG and pkg.hip.rtu_temporal_lambda_device(a._h, 2, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_lambda_device(None, 16, None) == pkg.RTU_ERR_ARG
        # free after rtu_destroy_context: the handle stays valid for that alone
        plain.close()
        held = pkg.hip.rtu_debug_device_bytes()
        c.close()
        assert pkg.hip.rtu_debug_device_bytes() < held - 248 * W * H + 1, "the session's buffers outlived the context"
        assert pkg.hip.rtu_temporal_lambda_device(a._h, 16, None) == pkg.RTU_ERR_ARG
        a.close()
    finally:
        c.close()
