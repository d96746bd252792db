"""GPU: steered sampling (include/rtu_render.h "Steered sampling"). The three device forms (rtu_sample_allocation_device,
rtu_extra_sample_rays_device, rtu_temporal_refine_device) against their host forms (which tests/test_steer_host.py holds to the
rules), bit for bit; a steered session's frames, plain and moved, against the same thing assembled by hand from the variance session's
host chain, the host forms and the existing ray-batch entries; the session's contract."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES
from test_gpu_ray_query import bits
from test_gpu_temporal import dev, orbit_frames
from test_gpu_temporal_motion import animated
from test_gpu_variance import ctx, fresh, same_bytes, variance_inputs  # noqa: F401 (ctx: a fixture)
from test_steer_host import BUDGETS, budget_of, lens_camera, odd_variance
from test_temporal_motion_host import table

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
ALL_SIZES = SIZES + [(200, 150)]  # 200 x 150: 30 scan tiles of 1024 pixels, the last of them partly filled


def steer_inputs(pkg, W, H):
    """Section 25's test history at this size with some pixels' history removed, the hits of its frame, and two variances."""
    hist, hits = variance_inputs(pkg, W, H)
    hist = hist.copy()
    valid = np.flatnonzero((hits["flags"] & 1) != 0)
    if W * H > 1:
        hist[0].reshape(-1, 4)[valid[1::7]] = 0.0
    return hist, hits, (pkg.variance(hist, hits), odd_variance(W, H, 7))


# ---- 1. the device forms against the host forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_allocation_device_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    stream = torch.cuda.Stream(device=0)
    hist, hits, vs = steer_inputs(pkg, W, H)
    d_hist, d_hits = dev(hist), dev(hits)
    first, spent, i = True, 0, 0
    for v in vs + (np.zeros((H, W), F),):
        d_v = dev(v)
        for bname in BUDGETS:
            for E, k in ((1, 0), (3, 7), (15, 0xffffffff)):
                i += 1
                desc = pkg.steer_desc(W, H, budget=budget_of(bname, W * H), max_extra=E, frame_index=k)
                wc, wo, wt = pkg.sample_allocation(hist, hits, v, desc)
                d_c, d_o, d_t = fresh(4 * W * H), fresh(4 * W * H), fresh(4)
                s = stream if i % 2 else None
                torch.cuda.synchronize()
                a0 = pkg.hip.rtu_debug_device_allocations()
                ctx.sample_allocation_device(desc, d_hist.data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), d_c.data_ptr(), d_o.data_ptr(), d_t.data_ptr(),
                                             s.cuda_stream if s else None)
                (s or torch.cuda).synchronize()
                assert first or pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated after its first call at this size"
                first = False
                assert same_bytes(d_hist, hist) and same_bytes(d_hits, hits) and same_bytes(d_v, v), "an input was written"
                gc, go, gt = d_c.cpu().numpy().view(U).reshape(H, W), d_o.cpu().numpy().view(U).reshape(H, W), int(d_t.cpu().numpy().view(U)[0])
                assert np.array_equal(gc, wc) and np.array_equal(go, wo) and gt == wt, (bname, E, k)
                spent += gt
    assert spent > 0 or size == (1, 1)


def test_allocation_device_with_more_tiles_than_scan_lanes(pkg, ctx):
    """640 x 421: 264 scan tiles, more than the 256 lanes of k_steer_sums, so a lane scans two tile sums and the last lanes none — the
    smallest size at which that kernel takes this path. Synthetic planes: only E.n, M.x, the hit flags and v are read."""
    import torch
    W, H = 640, 421
    n = W * H
    rng = np.random.default_rng(11)
    hist = np.zeros((4, H, W, 4), F)
    hist[0][..., 3] = np.where(rng.random((H, W)) < 0.1, 0.0, rng.integers(1, 33, (H, W))).astype(F)
    hist[3][..., 0] = rng.uniform(0.0, 0.5, (H, W)).astype(F)
    hits = np.zeros(n, pkg.hit_dtype())
    hits["flags"] = rng.choice(np.array([0, 1, 1, 1, 1, 1, 1, 2], np.uint32), n)
    v = (F(10.0) ** rng.uniform(-9, -2, (H, W))).astype(F)
    v[rng.random((H, W)) < 0.05] = np.nan
    d_hist, d_hits, d_v = dev(hist), dev(hits), dev(v)
    for budget, E, k in ((n // 4, 3, 5), (n, 1, 6), (4 * n, 15, 7)):
        desc = pkg.steer_desc(W, H, budget=budget, max_extra=E, frame_index=k)
        wc, wo, wt = pkg.sample_allocation(hist, hits, v, desc)
        d_c, d_o, d_t = fresh(4 * n), fresh(4 * n), fresh(4)
        ctx.sample_allocation_device(desc, d_hist.data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), d_c.data_ptr(), d_o.data_ptr(), d_t.data_ptr())
        torch.cuda.synchronize()
        gc, go, gt = d_c.cpu().numpy().view(U).reshape(H, W), d_o.cpu().numpy().view(U).reshape(H, W), int(d_t.cpu().numpy().view(U)[0])
        assert np.array_equal(gc, wc) and np.array_equal(go, wo) and gt == wt and gt > 1000, (budget, E, k)


@pytest.mark.parametrize("size", ALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_extra_rays_device_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    stream = torch.cuda.Stream(device=0)
    hist, hits, vs = steer_inputs(pkg, W, H)
    for i, (S, E, k, bname) in enumerate(((1, 1, 0, "pixels"), (4, 3, 6, "quarter"), (16, 15, 21, "four"), (4096, 15, 4100, "four"))):
        frame = lens_camera(pkg, W, H, S)
        desc = pkg.steer_desc(W, H, budget=budget_of(bname, W * H), max_extra=E, frame_index=k)
        counts, offsets, total = pkg.sample_allocation(hist, hits, vs[0], desc)
        rays, keys, owner = pkg.extra_sample_rays(frame, counts, offsets, desc)
        pad = 3  # the arrays are longer than the capacity: what lies beyond it stays as it was
        d_c, d_o = dev(counts), dev(offsets)
        d_rays, d_keys, d_owner = fresh(32 * (total + pad)), fresh(4 * (total + pad)), fresh(4 * (total + pad))
        s = stream if i % 2 else None
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.extra_sample_rays_device(desc, frame, d_c.data_ptr(), d_o.data_ptr(), total, d_rays.data_ptr(), d_keys.data_ptr(), d_owner.data_ptr(),
                                     s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        assert same_bytes(d_c, counts) and same_bytes(d_o, offsets), "an input was written"
        for what, d, w, size_of in (("rays", d_rays, rays, 32), ("keys", d_keys, keys, 4), ("owner", d_owner, owner, 4)):
            got = d.cpu().numpy()
            assert got[:size_of * total].tobytes() == w.tobytes(), "%s differ (%s)" % (what, (S, E, k, bname))
            assert (got[size_of * total:] == 0x5A).all(), "%s: written beyond the capacity" % what
        assert total > 0 or size == (1, 1)
    # a capacity below the total: the rays below it are the same, nothing at or beyond it is written
    if total > 4:
        cap = total - 3
        d_rays, d_keys, d_owner = fresh(32 * total), fresh(4 * total), fresh(4 * total)
        ctx.extra_sample_rays_device(desc, frame, d_c.data_ptr(), d_o.data_ptr(), cap, d_rays.data_ptr(), d_keys.data_ptr(), d_owner.data_ptr())
        torch.cuda.synchronize()
        got = d_rays.cpu().numpy()
        assert got[:32 * cap].tobytes() == rays[:cap].tobytes() and (got[32 * cap:] == 0x5A).all()
        assert (d_keys.cpu().numpy()[4 * cap:] == 0x5A).all() and (d_owner.cpu().numpy()[4 * cap:] == 0x5A).all()


@pytest.mark.parametrize("size", ALL_SIZES, ids=lambda s: "%dx%d" % s)
def test_refine_device_equals_the_host_form(pkg, ctx, size):
    import torch
    from test_temporal_host import chain_cameras, chain_inputs
    from test_variance_host import moments_chain
    W, H = size
    stream = torch.cuda.Stream(device=0)
    frames = chain_inputs(pkg, W, H, 4321)
    rgbz, hist0 = moments_chain(pkg, chain_cameras(pkg, W, H)["X"], frames, pkg.temporal_desc(W, H), table("static"), 0)[-1]
    hits, albedo = frames[-1][1], frames[-1][2]
    hist = hist0.copy()
    valid = np.flatnonzero((hits["flags"] & 1) != 0)
    if W * H > 1:
        hist[0].reshape(-1, 4)[valid[1::7]] = 0.0
    v = pkg.variance(hist, hits)
    d_hits, d_alb = dev(hits), dev(albedo)
    changed = 0
    for i, (bname, E, over) in enumerate((("four", 15, {}), ("pixels", 3, {"max_history": 3}), ("quarter", 1, {}), ("0", 3, {}))):
        counts, offsets, total = pkg.sample_allocation(hist, hits, v, pkg.steer_desc(W, H, budget=budget_of(bname, W * H), max_extra=E, frame_index=i))
        rng = np.random.default_rng(i)
        rgbt = rng.uniform(0.0, 2.0, (total, 4)).astype(F)
        if total > 8:
            rgbt[1, 0], rgbt[3, 2], rgbt[5, 1], rgbt[7, :3] = np.nan, np.inf, -np.inf, 1e20
        td = pkg.temporal_desc(W, H, **over)
        want_img, want_hist = pkg.temporal_refine(hist, rgbz, hits, albedo, counts, offsets, rgbt, td)
        d_hist, d_img, d_c, d_o = dev(hist), dev(rgbz), dev(counts), dev(offsets)
        d_rgbt = dev(rgbt) if total else fresh(16)
        s = stream if i % 2 else None
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.temporal_refine_device(td, d_hist.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_c.data_ptr(), d_o.data_ptr(), d_rgbt.data_ptr(), total,
                                   d_img.data_ptr(), s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        assert same_bytes(d_hits, hits) and same_bytes(d_alb, albedo) and same_bytes(d_c, counts) and same_bytes(d_o, offsets), "an input was written"
        assert total == 0 or same_bytes(d_rgbt, rgbt), "the samples were written"
        got_hist, got_img = d_hist.cpu().numpy().view(F).reshape(4, H, W, 4), d_img.cpu().numpy().view(F).reshape(H, W, 4)
        for what, g, w in (("image", got_img, want_img), ("history", got_hist, want_hist)):
            diff = bits(g) != bits(w)
            assert not diff.any(), "%s %s: %d words differ, first at %s" % ((bname, E, over), what, diff.sum(), np.argwhere(diff)[0])
        changed += int((bits(got_hist) != bits(hist)).sum())
    assert changed > 0 or size == (1, 1)


def test_device_refusals(pkg, ctx):
    import torch
    W, H = 7, 5
    n = W * H
    hist, hits, vs = steer_inputs(pkg, W, H)
    desc = pkg.steer_desc(W, H, budget=n, max_extra=3)
    counts, offsets, total = pkg.sample_allocation(hist, hits, vs[0], desc)
    d_hist, d_hits, d_v, d_c, d_o = dev(hist), dev(hits), dev(vs[0]), dev(counts), dev(offsets)
    buf = torch.zeros(4096 + 64 * n * 4, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    d_t, d_rays, d_keys, d_owner, d_rgbt, d_img, d_alb = base, base + 16, base + 16 + 32 * 4 * n, base + 16 + 36 * 4 * n, base + 16 + 40 * 4 * n, base + 16 + 56 * 4 * n, base + 16 + 60 * 4 * n
    frame = lens_camera(pkg, W, H, 4)
    ref = lambda d: ctypes.byref(d) if d is not None else None

    def alloc(d=desc, a=None):
        return pkg.hip.rtu_sample_allocation_device(ctx._h, ref(d), *(a or [d_hist.data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), d_c.data_ptr(), d_o.data_ptr(), d_t]), None)

    def rays(d=desc, f=frame, a=None, cap=total):
        a = a or [d_c.data_ptr(), d_o.data_ptr(), d_rays, d_keys, d_owner]
        return pkg.hip.rtu_extra_sample_rays_device(ctx._h, ref(d), ref(f), a[0], a[1], cap, a[2], a[3], a[4], None)

    td = pkg.temporal_desc(W, H)

    def fold(d=td, a=None, nr=total):
        a = a or [d_hist.data_ptr(), d_hits.data_ptr(), d_alb, d_c.data_ptr(), d_o.data_ptr(), d_rgbt, d_img]
        return pkg.hip.rtu_temporal_refine_device(ctx._h, ref(d), a[0], a[1], a[2], a[3], a[4], a[5], nr, a[6], None)

    assert alloc() == rays() == fold() == pkg.RTU_OK
    full = [d_hist.data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), d_c.data_ptr(), d_o.data_ptr(), d_t]
    for i in range(6):
        assert alloc(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
        assert alloc(a=[p + 2 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    assert alloc(a=[p + 4 if j == 0 else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG  # the history: 16-byte aligned
    full = [d_c.data_ptr(), d_o.data_ptr(), d_rays, d_keys, d_owner]
    for i in range(5):
        assert rays(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
        assert rays(a=[p + 2 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    assert rays(a=[p + 8 if j == 2 else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    assert rays(f=None) == rays(d=None) == rays(cap=(1 << 26) + 1) == pkg.RTU_ERR_ARG
    assert rays(f=lens_camera(pkg, W, H, 0)) == rays(f=lens_camera(pkg, W, H, 16385)) == rays(f=lens_camera(pkg, W + 1, H, 4)) == pkg.RTU_ERR_ARG
    full = [d_hist.data_ptr(), d_hits.data_ptr(), d_alb, d_c.data_ptr(), d_o.data_ptr(), d_rgbt, d_img]
    for i in range(7):
        assert fold(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
        assert fold(a=[p + 2 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    assert fold(d=None) == fold(nr=(1 << 26) + 1) == fold(d=pkg.temporal_desc(W, H, max_history=0)) == pkg.RTU_ERR_ARG
    for bad in ({"max_extra": 0}, {"max_extra": 16}, {"budget": (1 << 26) + 1}, {"width": 0}, {"height": 65537}):
        bd = pkg.steer_desc(W, H, budget=n)
        for k, x in bad.items():
            setattr(bd, k, x)
        assert alloc(d=bd) == pkg.RTU_ERR_ARG and rays(d=bd) == pkg.RTU_ERR_ARG, bad
    bd = pkg.steer_desc(W, H, budget=n)
    bd.reserved[1] = 1
    assert alloc(d=bd) == rays(d=bd) == alloc(d=None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_sample_allocation_device(None, ref(desc), d_hist.data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), d_c.data_ptr(), d_o.data_ptr(), d_t, None) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()


# ---- 2. sessions against the hand-assembled form ------------------------------------------------------------------------------------
def hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, sdesc, motion, cap):
    """Frame k by existing entries and the host forms: the variance session's host chain (host rays -> host shading -> frame_features
    -> host moments accumulator -> host variance), then host allocation -> host extra rays -> the existing ray-batch shading -> host
    fold -> host variance -> host filter."""
    rays, keys = pkg.camera_sample_rays(frame, k % frame.samples)
    shade = ctx.shade_rays_paths if frame.gather_bounces else ctx.shade_rays_sampled
    rgbt = shade(rays, keys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0].reshape(frame.height, frame.width, 4)
    hits, albedo = ctx.frame_features(frame)
    out, hist = pkg.temporal_accumulate_moments(prev, frame, rgbt, hits, albedo, motion, hist, desc, cap)
    v = pkg.variance(hist, hits, vdesc)
    sd = pkg.steer_desc(frame.width, frame.height, budget=sdesc.budget, max_extra=sdesc.max_extra, frame_index=k)
    counts, offsets, total = pkg.sample_allocation(hist, hits, v, sd)
    if total:
        xrays, xkeys, owner = pkg.extra_sample_rays(frame, counts, offsets, sd)
        xrgbt = shade(xrays, xkeys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0]
        out, hist = pkg.temporal_refine(hist, out, hits, albedo, counts, offsets, xrgbt, desc)
        v = pkg.variance(hist, hits, vdesc)
    return pkg.denoise_variance(out, hits, albedo, v, vdesc), hist, hits, counts, total


@pytest.mark.parametrize("tag,kw,distance", [("p10_s4_160x120", {"samples": 3}, 20.0), ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0)],
                         ids=["S", "P"])
def test_session_equals_the_hand_form(pkg, ctx, golden, tag, kw, distance):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    frames = orbit_frames(pkg, scene, W, H, 3, distance, 0.5, **kw)  # a moving camera
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    sdesc = pkg.steer_desc(budget=W * H // 2, max_extra=3)
    still = table("static", scene.desc.n_nodes)
    s = ctx.temporal(desc, variance=pkg.variance_desc(), steer=sdesc)
    plain = ctx.temporal(desc, variance=pkg.variance_desc())
    try:
        assert not s.extra_counts().any() and s.steer_total() == 0
        prev = hist = None
        spent = differs = 0
        for k, frame in enumerate(frames):
            got = s.frame(frame)
            want, hist, hits, counts, total = hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, sdesc, still, 0)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3]))
            assert np.array_equal(s.extra_counts(), counts) and s.steer_total() == total
            spent += total
            differs += int((bits(got) != bits(plain.frame(frame))).sum())
        assert spent >= 0.5 * 3 * (W * H // 2), "the budget was not spent: %d rays" % spent
        assert differs > 0, "the extra rays changed nothing"
    finally:
        s.close()
        plain.close()


def test_moved_session_equals_the_hand_form(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    W, H = g.width, g.height
    scenes = animated(pkg, g.scene(pkg), 2, 20.0, 0.2)
    frames = [pkg.frame_setup(sc.desc.camera, W, H, samples=3) for sc in scenes]
    ctx.upload(scenes[0])
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    sdesc = pkg.steer_desc(budget=W * H, max_extra=2)
    s = ctx.temporal(desc, variance=vdesc, steer=sdesc)
    try:
        prev = hist = None
        for k, frame in enumerate(frames):
            if k:
                ctx.update(scenes[k])  # rtu_update_scene
            motion = pkg.scene_motion(scenes[k - 1] if k else scenes[0], scenes[k])
            want, hist, hits, counts, total = hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, sdesc, motion, 3)
            got = s.frame_moved(frame, motion, 3)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3])) and np.array_equal(s.extra_counts(), counts) and total > 0
    finally:
        s.close()


# ---- 3. the contract ---------------------------------------------------------------------------------------------------------------
def test_session_contract(pkg, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    frames = orbit_frames(pkg, scene, W, H, 3, 20.0, 0.5, samples=4)
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc()
    c = pkg.Context(0)
    try:
        a = c.temporal(desc, variance=vdesc, steer=pkg.steer_desc(budget=W * H // 4, max_extra=3))
        with pytest.raises(pkg.RtuError) as e:      # before an upload
            a.frame(frames[0])
        assert e.value.code == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        plain = c.temporal(desc, variance=vdesc)    # a plain variance session on the same context: its bits
        plain_want = [plain.frame(f) for f in frames]
        plain.close()
        zero = c.temporal(desc, variance=vdesc, steer=pkg.steer_desc(budget=0, max_extra=3))
        plain = c.temporal(desc, variance=vdesc)
        for k, f in enumerate(frames):
            a0 = pkg.hip.rtu_debug_device_allocations()
            got = a.frame(f)
            assert k == 0 or pkg.hip.rtu_debug_device_allocations() == a0, "frame %d of a steered session allocated" % k
            assert a.steer_total() > 0 and int(a.extra_counts().sum()) == a.steer_total() <= W * H // 4
            assert (bits(got) != bits(plain_want[k])).any(), "the extra rays changed nothing"
            # budget 0: a variance session's bits; a plain variance session between the steered frames keeps its bits
            assert np.array_equal(bits(zero.frame(f)), bits(plain_want[k])) and zero.steer_total() == 0 and not zero.extra_counts().any()
            assert np.array_equal(bits(plain.frame(f)), bits(plain_want[k])), "a steered session changed a variance session's frame"
        a.reset()
        assert a.steer_total() == 0 and not a.extra_counts().any() and not a.history().any()
        # the refusals
        for over in ({"max_extra": 0}, {"max_extra": 16}, {"budget": (1 << 26) + 1}):
            with pytest.raises(pkg.RtuError) as e:
                c.temporal(desc, variance=vdesc, steer=pkg.steer_desc(**over))
            assert e.value.code == pkg.RTU_ERR_ARG, over
        bd = pkg.steer_desc(budget=5)
        bd.reserved[0] = 1
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=vdesc, steer=bd)
        with pytest.raises(pkg.RtuError):
            c.temporal(pkg.temporal_desc(W, H, denoise=True), variance=vdesc, steer=pkg.steer_desc(budget=5))
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=pkg.variance_desc(n_passes=0), steer=pkg.steer_desc(budget=5))
        err = ctypes.c_int(0)
        sd = pkg.steer_desc(budget=5)
        assert not pkg.hip.rtu_temporal_begin_steered(None, ctypes.byref(desc), ctypes.byref(vdesc), ctypes.byref(sd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not pkg.hip.rtu_temporal_begin_steered(c._h, ctypes.byref(desc), ctypes.byref(vdesc), None, ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not pkg.hip.rtu_temporal_begin_steered(c._h, ctypes.byref(desc), None, ctypes.byref(sd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not pkg.hip.rtu_temporal_begin_steered(c._h, None, ctypes.byref(vdesc), ctypes.byref(sd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        with pytest.raises(pkg.RtuError) as e:      # S * (1 + E) > 65536
            a.frame(pkg.frame_setup(scene.desc.camera, W, H, samples=16385))
        assert e.value.code == pkg.RTU_ERR_ARG
        with pytest.raises(pkg.RtuError):           # not a steered session
            plain.extra_counts()
        with pytest.raises(pkg.RtuError):
            plain.steer_total()
        n = ctypes.c_uint32(0)
        assert pkg.hip.rtu_temporal_steer_total(a._h, None) == pkg.RTU_ERR_ARG and pkg.hip.rtu_temporal_extra_counts_device(a._h, None, None) == pkg.RTU_ERR_ARG
        # free after rtu_destroy_context: the handles stay valid for that alone
        plain.close()
        held = pkg.hip.rtu_debug_device_bytes()
        c.close()
        assert pkg.hip.rtu_debug_device_bytes() < held - 2 * 248 * W * H + 1, "the sessions' buffers outlived the context"
        assert pkg.hip.rtu_temporal_steer_total(a._h, ctypes.byref(n)) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_extra_counts_device(a._h, 16, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_frame(a._h, ctypes.byref(frames[0]), np.empty((H, W, 4), F).ctypes.data) == pkg.RTU_ERR_ARG
        a.close()
        zero.close()
    finally:
        c.close()
