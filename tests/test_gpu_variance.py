"""GPU: variance-guided filtering (include/rtu_render.h "Variance-guided filtering"). The three device forms
(rtu_temporal_accumulate_moments_device, rtu_variance_device, rtu_denoise_variance_device) against their host forms (which
tests/test_variance_host.py holds to the rules), bit for bit; a variance session's frames, plain and moved, against the same thing
assembled by hand from existing entries and the host forms; the session's contract."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES, make_inputs
from test_gpu_ray_query import bits
from test_gpu_temporal import dev, orbit_frames
from test_gpu_temporal_motion import MESH_NODE, SPHERE_NODE, animated
from test_temporal_host import FRAMES, chain_cameras, chain_inputs
from test_temporal_motion_host import CASES, STATIC, case_cameras, table
from test_variance_host import FILTER_SETS, VARIANCE_SETS, make_variance, moments_chain

pytestmark = pytest.mark.gpu

F = np.float32


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def fresh(nbytes):
    import torch
    return torch.full((nbytes,), 0x5A, dtype=torch.uint8, device="cuda:0")


def same_bytes(d, a):
    return np.array_equal(d.cpu().numpy(), np.ascontiguousarray(a).view(np.uint8).reshape(-1))


# ---- 1. the device forms against the host forms --------------------------------------------------------------------------------------
def device_moments_chain(pkg, ctx, cams, frames, desc, motion, cap, streams, in_place_at):
    import torch
    res, d_prev, hist = [], None, None
    for k in range(len(frames)):
        rgbz, hits, albedo = frames[k]
        H, W = rgbz.shape[:2]
        d_in, d_hits, d_alb = dev(rgbz), dev(hits), dev(albedo)
        d_motion = dev(motion) if len(motion) else fresh(96)  # (an empty table still needs a pointer)
        d_hist = fresh(4 * H * W * 16)
        in_place = k == in_place_at
        d_out = d_in if in_place else fresh(H * W * 16)
        s = streams[k % 2]
        table_before = d_motion.cpu().numpy()
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.temporal_accumulate_moments_device(desc, cams[k - 1] if k else None, cams[k], d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                               d_prev.data_ptr() if d_prev is not None else None, d_hist.data_ptr(), d_out.data_ptr(),
                                               d_motion.data_ptr(), len(motion), cap, s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        assert in_place or same_bytes(d_in, rgbz), "the input was written"
        assert same_bytes(d_hits, hits) and same_bytes(d_alb, albedo), "a guide was written"
        assert np.array_equal(d_motion.cpu().numpy(), table_before), "the table was written"
        assert d_prev is None or same_bytes(d_prev, hist), "the previous history was written"
        hist = d_hist.cpu().numpy().view(F).reshape(4, H, W, 4)
        res.append((d_out.cpu().numpy().view(F).reshape(H, W, 4), hist))
        d_prev = d_hist
    return res


def compare_moments(pkg, ctx, stream, W, H, ci, case):
    kind, n, camname, cap, over = case
    cams = case_cameras(pkg, W, H, camname)
    frames = chain_inputs(pkg, W, H, 1234 + ci)
    desc = pkg.temporal_desc(W, H, **over)
    motion = table(kind)[:n]
    want = moments_chain(pkg, cams, frames, desc, motion, cap)
    got = device_moments_chain(pkg, ctx, cams, frames, desc, motion, cap, (None, stream), in_place_at=1 + ci % 4)
    for k in range(FRAMES):
        for what, g, w in (("image", got[k][0], want[k][0]), ("history", got[k][1], want[k][1])):
            diff = bits(g) != bits(w)
            assert not diff.any(), "table %s[%d] cameras %s cap %d %s frame %d %s: %d words differ, first at %s" % (
                kind, n, camname, cap, over, k, what, diff.sum(), np.argwhere(diff)[0])
    return want


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_moments_device_equals_the_host_form(pkg, ctx, size):
    import torch
    stream = torch.cuda.Stream(device=0)
    grown = False
    for ci, case in enumerate(CASES):
        want = compare_moments(pkg, ctx, stream, size[0], size[1], ci, case)
        grown |= bool((want[-1][1][3][..., 0] != 0).any() and (want[-1][1][0][..., 3] > 1).any())
    assert grown or size == (1, 1), "nothing was accumulated"


def test_moments_device_equals_the_host_form_at_200x150(pkg, ctx):
    """More than one workgroup in both directions, neither a multiple of the 32 x 8 tile; the case that mixes one-tap and reprojecting
    lanes in one wavefront, and the one that normalises."""
    import torch
    stream = torch.cuda.Stream(device=0)
    for ci in (3, 5):
        compare_moments(pkg, ctx, stream, 200, 150, ci, CASES[ci])


def variance_inputs(pkg, W, H):
    frames = chain_inputs(pkg, W, H, 4321)
    hist = moments_chain(pkg, chain_cameras(pkg, W, H)["X"], frames, pkg.temporal_desc(W, H), table("static"), 0)[-1][1]
    return np.ascontiguousarray(hist), frames[-1][1]


@pytest.mark.parametrize("size", SIZES + [(200, 150)], ids=lambda s: "%dx%d" % s)
def test_variance_device_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    stream = torch.cuda.Stream(device=0)
    hist, hits = variance_inputs(pkg, W, H)
    d_hist, d_hits = dev(hist), dev(hits)
    short = 0
    for k, over in enumerate(VARIANCE_SETS):
        desc = pkg.variance_desc(W, H, **over)
        want = pkg.variance(hist, hits, desc)
        d_v = fresh(H * W * 4)
        s = stream if k % 2 else None
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.variance_device(desc, d_hist.data_ptr(), d_hits.data_ptr(), d_v.data_ptr(), s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        assert same_bytes(d_hist, hist) and same_bytes(d_hits, hits), "an input was written"
        got = d_v.cpu().numpy().view(F).reshape(H, W)
        diff = bits(got) != bits(want)
        assert not diff.any(), "%s: %d words differ, first at %s" % (over, diff.sum(), np.argwhere(diff)[0])
        n = hist[0][..., 3]
        short += int(((n > 0) & (n < desc.min_history)).sum())
    assert short > 0


@pytest.mark.parametrize("size", SIZES + [(200, 150)], ids=lambda s: "%dx%d" % s)
def test_filter_device_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    stream = torch.cuda.Stream(device=0)
    rgbz, hits, albedo = make_inputs(pkg, W, H, 1234 + len(SIZES))
    v = make_variance(W, H, 7)
    d_hits, d_alb, d_v = dev(hits), dev(albedo), dev(v)
    first = True
    for n_passes in ((1, 2, 3, 6) if size != (200, 150) else (3, 5)):  # the step exceeds the small images
        for j, over in enumerate(FILTER_SETS):
            desc = pkg.variance_desc(W, H, n_passes=n_passes, **over)
            want = pkg.denoise_variance(rgbz, hits, albedo, v, desc)
            d_in = dev(rgbz)
            in_place = (n_passes + j) % 2 == 0
            d_out = d_in if in_place else fresh(H * W * 16)
            s = stream if j % 2 else None
            torch.cuda.synchronize()
            a0 = pkg.hip.rtu_debug_device_allocations()
            ctx.denoise_variance_device(desc, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_v.data_ptr(), d_out.data_ptr(), s.cuda_stream if s else None)
            (s or torch.cuda).synchronize()
            assert first or pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated after its first call at this size"
            first = False
            assert in_place or same_bytes(d_in, rgbz), "the input was written"
            assert same_bytes(d_hits, hits) and same_bytes(d_alb, albedo) and same_bytes(d_v, v), "a guide was written"
            got = d_out.cpu().numpy().view(F).reshape(H, W, 4)
            diff = bits(got) != bits(want)
            assert not diff.any(), "%d passes %s: %d words differ, first at %s" % (n_passes, over, diff.sum(), np.argwhere(diff)[0])


def test_device_refusals(pkg, ctx):
    import torch
    W, H = 7, 5
    n = W * H
    buf = torch.zeros(n * 400 + 3 * 96 + 64, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    # rgbz, hits, albedo, hist_prev, hist_out, out, table; then v
    ptrs = [base, base + 16 * n, base + 64 * n, base + 80 * n, base + 144 * n, base + 208 * n, base + 224 * n]
    d_v = base + 224 * n + 3 * 96
    buf[224 * n:224 * n + 3 * 96] = torch.from_numpy(table("slide").view(np.uint8).copy()).to("cuda:0")
    cams = chain_cameras(pkg, W, H)["X"]
    d = pkg.temporal_desc(W, H)

    def acc(desc=d, p=ptrs, prev=cams[2], cur=cams[3], nn=3, cap=2):
        return pkg.hip.rtu_temporal_accumulate_moments_device(ctx._h, ctypes.byref(desc), ctypes.byref(prev) if prev is not None else None,
                                                              ctypes.byref(cur) if cur is not None else None, *p, nn, cap, None)
    assert acc() == pkg.RTU_OK
    for k in range(7):
        p = list(ptrs)
        p[k] = None
        assert acc(p=p, prev=None if k == 3 else cams[2]) == (pkg.RTU_OK if k == 3 else pkg.RTU_ERR_ARG), k
        p[k] = ptrs[k] + 8
        assert acc(p=p) == pkg.RTU_ERR_ARG, k
    p = list(ptrs)
    p[4] = ptrs[3] + 64 * n - 16        # the last pixel of the previous M overlaps the new E
    assert acc(p=p) == pkg.RTU_ERR_ARG
    for cap in (-1, 65536):
        assert acc(cap=cap) == pkg.RTU_ERR_ARG
    assert acc(desc=pkg.temporal_desc(W, H, max_history=0)) == pkg.RTU_ERR_ARG and acc(desc=pkg.temporal_desc(W + 1, H)) == pkg.RTU_ERR_ARG
    assert acc(cur=None) == pkg.RTU_ERR_ARG and acc(prev=None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_temporal_accumulate_moments_device(None, ctypes.byref(d), ctypes.byref(cams[2]), ctypes.byref(cams[3]), *ptrs, 3, 0, None) == pkg.RTU_ERR_ARG

    vd = pkg.variance_desc(W, H)
    var = lambda desc=vd, hist=ptrs[4], hits=ptrs[1], v=d_v: pkg.hip.rtu_variance_device(ctx._h, ctypes.byref(desc) if desc is not None else None, hist, hits, v, None)
    flt = lambda desc=vd, a=ptrs[0], hits=ptrs[1], alb=ptrs[2], v=d_v, out=ptrs[5]: pkg.hip.rtu_denoise_variance_device(
        ctx._h, ctypes.byref(desc) if desc is not None else None, a, hits, alb, v, out, None)
    assert var() == pkg.RTU_OK and flt() == pkg.RTU_OK
    assert var(desc=None) == var(hist=None) == var(hits=None) == var(v=None) == var(hist=ptrs[4] + 8) == var(hits=ptrs[1] + 4) == var(v=d_v + 2) == pkg.RTU_ERR_ARG
    assert flt(desc=None) == flt(a=None) == flt(hits=None) == flt(alb=None) == flt(v=None) == flt(out=None) == pkg.RTU_ERR_ARG
    assert flt(a=ptrs[0] + 8) == flt(hits=ptrs[1] + 8) == flt(alb=ptrs[2] + 4) == flt(out=ptrs[5] + 8) == flt(v=d_v + 1) == pkg.RTU_ERR_ARG
    assert var(v=d_v + 4) == pkg.RTU_OK and flt(v=d_v + 4) == pkg.RTU_OK  # v is floats: 4-byte aligned
    for bad in ({"n_passes": 0}, {"n_passes": 9}, {"sigma_lum": 0.0}, {"sigma_plane": float("nan")}, {"normal_log2_power": 8}, {"min_history": 0},
                {"min_history": 65536}, {"width": 0}, {"height": 65537}):
        bd = pkg.variance_desc(W, H)
        for k, x in bad.items():
            setattr(bd, k, x)
        assert var(desc=bd) == pkg.RTU_ERR_ARG and flt(desc=bd) == pkg.RTU_ERR_ARG, bad
    for k in range(3):
        bd = pkg.variance_desc(W, H)
        bd.reserved[k] = 1
        assert var(desc=bd) == pkg.RTU_ERR_ARG and flt(desc=bd) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_variance_device(None, ctypes.byref(vd), ptrs[4], ptrs[1], d_v, None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_denoise_variance_device(None, ctypes.byref(vd), ptrs[0], ptrs[1], ptrs[2], d_v, ptrs[5], None) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()


# ---- 2. sessions against the hand-assembled form ------------------------------------------------------------------------------------
def hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, motion, cap):
    """Frame k by existing entries and the host forms: host rays -> host shading -> frame_features -> host moments accumulator -> host
    variance -> host filter."""
    rays, keys = pkg.camera_sample_rays(frame, k % frame.samples)
    shade = ctx.shade_rays_paths if frame.gather_bounces else ctx.shade_rays_sampled
    rgbt = shade(rays, keys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0].reshape(frame.height, frame.width, 4)
    hits, albedo = ctx.frame_features(frame)
    out, hist = pkg.temporal_accumulate_moments(prev, frame, rgbt, hits, albedo, motion, hist, desc, cap)
    v = pkg.variance(hist, hits, vdesc)
    return pkg.denoise_variance(out, hits, albedo, v, vdesc), hist, hits, out


@pytest.mark.parametrize("tag,kw,distance", [("p10_s4_160x120", {"samples": 3}, 20.0), ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0)],
                         ids=["S", "P"])
def test_session_equals_the_hand_form(pkg, ctx, golden, tag, kw, distance):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    frames = orbit_frames(pkg, scene, W, H, 4, distance, 0.5, **kw)  # a moving camera; samples 0, 1, 2, 0 of S = 3
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    still = table("static", scene.desc.n_nodes)  # what a plain frame of a variance session uses
    s = ctx.temporal(desc, variance=pkg.variance_desc())  # (the session takes its own size)
    try:
        assert not s.history().any()
        prev = hist = None
        changed = 0
        for k, frame in enumerate(frames):
            got = s.frame(frame)
            want, hist, hits, unfiltered = hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, still, 0)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3]))
            changed += int((bits(want) != bits(unfiltered)).sum())
        valid = (hits["flags"] & 1) != 0
        n = hist[0][..., 3].reshape(-1)
        assert (n[valid] > 1).mean() > 0.5 and n.max() > 3, "the camera's moves left no history to speak of"
        assert changed > 0, "the filter changed nothing"
    finally:
        s.close()


def test_moved_session_equals_the_hand_form(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    W, H = g.width, g.height
    scenes = animated(pkg, g.scene(pkg), 3, 20.0, 0.2)
    frames = [pkg.frame_setup(sc.desc.camera, W, H, samples=3) for sc in scenes]
    n_nodes = scenes[0].desc.n_nodes
    ctx.upload(scenes[0])
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H, n_passes=2, min_history=2)
    s = ctx.temporal(desc, variance=vdesc)
    try:
        prev = hist = None
        for k, frame in enumerate(frames):
            if k:
                ctx.update(scenes[k])
            motion = pkg.scene_motion(scenes[k - 1] if k else scenes[0], scenes[k])  # rtu_scene_motion
            assert k == 0 or [i for i in range(n_nodes) if not motion["flags"][i] & STATIC] == [MESH_NODE, SPHERE_NODE]
            moved = k != 1  # frame 1 is a plain frame: after the update it starts over, as in any session
            if not moved:
                prev = hist = None
            want, hist, hits, _ = hand_frame(pkg, ctx, frame, 0 if not moved else (k if k == 0 else k - 1), prev, hist, desc, vdesc,
                                             motion if moved else table("static", n_nodes), 3 if moved else 0)
            a0 = pkg.hip.rtu_debug_device_allocations()
            got = s.frame_moved(frame, motion, 3) if moved else s.frame(frame)
            assert k < 2 or pkg.hip.rtu_debug_device_allocations() == a0, "frame %d allocated" % k
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3]))
        valid = ((hits["flags"] & 1) != 0).reshape(H, W)
        n = s.history()
        moved_px = valid & np.isin(hits["node"].reshape(H, W), (MESH_NODE, SPHERE_NODE))
        assert (n[valid] > 1).mean() > 0.5 and moved_px.sum() > 100 and (n[moved_px] > 1).mean() > 0.5, "the moved nodes kept no history"
    finally:
        s.close()


# ---- 3. the contract ---------------------------------------------------------------------------------------------------------------
def test_session_contract(pkg, golden):
    import torch
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    frames = orbit_frames(pkg, scene, W, H, 3, 20.0, 0.5, samples=4)
    plain = pkg.frame_setup(scene.desc.camera, W, H, samples=2)
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc()
    c = pkg.Context(0)
    try:
        a = c.temporal(desc, variance=vdesc)
        with pytest.raises(pkg.RtuError) as e:      # before an upload
            a.frame(frames[0])
        assert e.value.code == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        old = c.temporal(desc)                      # a plain session on the same context: its old bits
        old_want = [old.frame(f) for f in frames[:2]]
        old.close()
        render0 = c.render(plain)[0]
        b = c.temporal(desc, variance=vdesc)
        old = c.temporal(desc)
        a0 = a.frame(frames[0])
        assert np.array_equal(bits(old.frame(frames[0])), bits(old_want[0]))
        a1 = a.frame(frames[1])
        b0 = b.frame(frames[0])
        between = c.render(plain)[0]                # a render between two frames of b ...
        n1 = pkg.hip.rtu_debug_device_allocations()
        b1 = b.frame(frames[1])
        assert pkg.hip.rtu_debug_device_allocations() == n1, "a frame after the first allocated"
        assert np.array_equal(bits(old.frame(frames[1])), bits(old_want[1])), "a variance session changed a plain session's frame"
        assert np.array_equal(bits(between), bits(render0)), "the session changed a render"
        assert np.array_equal(bits(b0), bits(a0)) and np.array_equal(bits(b1), bits(a1)), "the render changed the session's next frame"
        assert (bits(a1) != bits(old_want[1])).any(), "the variance session did not filter"
        # the device form on a caller's stream, and reset
        b.reset()
        assert not b.history().any()
        d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.Stream(device=0)
        c._check(pkg.hip.rtu_context_sync(c._h))
        b.frame_device(frames[0], d_out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert np.array_equal(bits(d_out.cpu().numpy()), bits(a0))
        # the refusals
        with pytest.raises(pkg.RtuError) as e:
            c.temporal(pkg.temporal_desc(W, H, denoise=True), variance=vdesc)
        assert e.value.code == pkg.RTU_ERR_ARG
        for over in ({"n_passes": 0}, {"n_passes": 9}, {"sigma_lum": 0.0}, {"sigma_plane": -1.0}, {"normal_log2_power": 8}, {"min_history": 0}):
            with pytest.raises(pkg.RtuError) as e:
                c.temporal(desc, variance=pkg.variance_desc(**over))
            assert e.value.code == pkg.RTU_ERR_ARG, over
        bd = pkg.variance_desc()
        bd.reserved[2] = 1
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=bd)
        with pytest.raises(pkg.RtuError):
            c.temporal(pkg.temporal_desc(W, H, flags=2), variance=vdesc)
        err = ctypes.c_int(0)
        assert not pkg.hip.rtu_temporal_begin_variance(None, ctypes.byref(desc), ctypes.byref(vdesc), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not pkg.hip.rtu_temporal_begin_variance(c._h, ctypes.byref(desc), None, ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not pkg.hip.rtu_temporal_begin_variance(c._h, None, ctypes.byref(vdesc), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        for bad in (pkg.frame_setup(scene.desc.camera, W + 1, H, samples=4), pkg.frame_setup(scene.desc.camera, W, H),
                    pkg.frame_setup(scene.desc.camera, W, H, shard_rank=0, shard_count=2, samples=4)):
            with pytest.raises(pkg.RtuError) as e:
                a.frame(bad)
            assert e.value.code == pkg.RTU_ERR_ARG
        # free after rtu_destroy_context: the handles stay valid for that alone
        old.close()
        held = pkg.hip.rtu_debug_device_bytes()
        c.close()
        assert pkg.hip.rtu_debug_device_bytes() < held - 2 * 248 * W * H + 1, "the sessions' buffers outlived the context"
        assert pkg.hip.rtu_temporal_frame(a._h, ctypes.byref(frames[0]), a0.ctypes.data) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_reset(a._h) == pkg.RTU_ERR_ARG
        a.close()
        b.close()
    finally:
        c.close()
