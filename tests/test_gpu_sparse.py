"""GPU: sparse sessions (include/rtu_render.h "Sparse sessions"). The three device forms (rtu_sparse_rays_device,
rtu_temporal_accumulate_sparse_device, rtu_sparse_fill_device) against their host forms (which tests/test_sparse_host.py holds to the
rules), bit for bit; a sparse session's frames, plain and moved, against the same steps assembled by hand from the host forms; the
session's contract."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES
from test_gpu_ray_query import bits
from test_gpu_temporal import dev, orbit_frames
from test_gpu_temporal_motion import animated
from test_gpu_variance import ctx, fresh, same_bytes  # noqa: F401 (ctx: a fixture)
from test_sparse_host import BLOCKS, grid, owners_of, sparse_inputs
from test_steer_host import lens_camera
from test_temporal_motion_host import table
from test_variance_host import all_chains

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
GPU_SIZES = SIZES + [(200, 150)]  # more than one workgroup in both directions, partial blocks at B = 3 (in x and y) and B = 4 (in y)
PAD = 16


def back(d, dtype, shape):
    return d.cpu().numpy().view(dtype).reshape(shape)


def padded(a):
    """`a` on the device with PAD guard bytes behind it."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = fresh(len(raw) + PAD)
    d[:len(raw)].copy_(torch.from_numpy(raw.copy()))
    return d


# ---- 1. the device forms against the host forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("size", GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_sparse_rays_device_equals_the_host_form(pkg, ctx, size, B):
    import torch
    W, H = size
    sw, sh = grid(W, H, B)
    m = sw * sh
    stream = torch.cuda.Stream(device=0)
    for i, (S, k) in enumerate(((1, 0), (16, 1), (3, B * B), (4096, 0xffffffff), (16, 7 * B * B + 3))):
        frame = lens_camera(pkg, W, H, S)
        sd = pkg.sparse_desc(W, H, block=B, frame_index=k)
        rays, keys, owner = pkg.sparse_rays(frame, sd)
        d_rays, d_keys, d_owner = fresh(32 * m + PAD), fresh(4 * m + PAD), fresh(4 * m + PAD)
        s = stream if i % 2 else None
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.sparse_rays_device(sd, frame, d_rays.data_ptr(), d_keys.data_ptr(), d_owner.data_ptr(), s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        for what, d, w, size_of in (("rays", d_rays, rays, 32), ("keys", d_keys, keys, 4), ("owner", d_owner, owner, 4)):
            got = d.cpu().numpy()
            assert got[:size_of * m].tobytes() == w.tobytes(), "%s differ (%s)" % (what, (S, k))
            assert (got[size_of * m:] == 0x5A).all(), "%s: written beyond the blocks" % what


@pytest.mark.parametrize("B", BLOCKS)
@pytest.mark.parametrize("size", GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_accumulator_and_fill_device_equal_the_host_forms(pkg, ctx, size, B):
    """The sparse accumulator and the fill along the chains of tests/test_sparse_host.py, with their NaN, infinite and overflowing
    samples at owners; every frame goes on from the host form's history."""
    import torch
    W, H = size
    n = W * H
    streams = (None, torch.cuda.Stream(device=0))
    sd = pkg.sparse_desc(W, H, block=B)
    chains = list(all_chains(pkg, W, H))
    holes = filled = 0
    for ci, (what, cams, frames, desc, motion, cap) in enumerate(chains if n < 10000 else chains[1::5]):
        d_motion = dev(motion) if len(motion) else fresh(96)
        hist = None
        for k, (rgbz, hits, albedo) in enumerate(frames):
            owner = owners_of(W, H, B, k)
            rgbt, _ = sparse_inputs(rgbz, owner, k)
            prev = cams[k - 1] if k else None
            want, want_hist, want_hole = pkg.temporal_accumulate_sparse(prev, cams[k], rgbt, owner, hits, albedo, motion, hist, desc, sd, cap)
            want_fill = pkg.sparse_fill(want, want_hole, hits, albedo, owner, rgbt, desc, sd)
            d_rgbt, d_owner, d_hits, d_alb = dev(rgbt), dev(owner), dev(hits), dev(albedo)
            d_prev = dev(hist) if hist is not None else None
            d_hist, d_out, d_hole = fresh(64 * n + PAD), fresh(16 * n + PAD), fresh(n + PAD)
            s = streams[(k + ci) % 2]
            torch.cuda.synchronize()
            a0 = pkg.hip.rtu_debug_device_allocations()
            ctx.temporal_accumulate_sparse_device(desc, sd, prev, cams[k], d_rgbt.data_ptr(), d_owner.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                                  d_prev.data_ptr() if d_prev is not None else None, d_hist.data_ptr(), d_out.data_ptr(),
                                                  d_hole.data_ptr(), d_motion.data_ptr(), len(motion), cap, s.cuda_stream if s else None)
            (s or torch.cuda).synchronize()
            assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
            where = "%s frame %d" % (what, k)
            g_out, g_hist, g_hole = d_out.cpu().numpy(), d_hist.cpu().numpy(), d_hole.cpu().numpy()
            for name, g, w in (("image", g_out, want), ("history", g_hist, want_hist), ("hole", g_hole, want_hole)):
                wb = np.ascontiguousarray(w).view(np.uint8).reshape(-1)
                bad = g[:len(wb)] != wb
                assert not bad.any(), "%s %s: %d bytes differ, first at %d" % (where, name, bad.sum(), np.flatnonzero(bad)[0])
                assert (g[len(wb):] == 0x5A).all(), "%s %s: written beyond the pixels" % (where, name)
            # the fill, in place in a copy of the host form's image
            d_img, d_h = padded(want), dev(want_hole)
            torch.cuda.synchronize()
            a0 = pkg.hip.rtu_debug_device_allocations()
            ctx.sparse_fill_device(desc, sd, d_hits.data_ptr(), d_alb.data_ptr(), d_owner.data_ptr(), d_rgbt.data_ptr(), d_h.data_ptr(), d_img.data_ptr(),
                                   s.cuda_stream if s else None)
            (s or torch.cuda).synchronize()
            assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
            g = d_img.cpu().numpy()
            bad = bits(g[:16 * n].view(F).reshape(H, W, 4)) != bits(want_fill)
            assert not bad.any(), "%s fill: %d words differ, first at %s" % (where, bad.sum(), np.argwhere(bad)[0])
            assert (g[16 * n:] == 0x5A).all(), "%s fill: written beyond the pixels" % where
            assert same_bytes(d_rgbt, rgbt) and same_bytes(d_owner, owner) and same_bytes(d_hits, hits) and same_bytes(d_alb, albedo) and \
                same_bytes(d_h, want_hole), "an input was written"
            assert d_prev is None or same_bytes(d_prev, hist), "an input was written"
            holes += int(want_hole.sum())
            filled += int((bits(want_fill) != bits(want)).any(-1).sum())
            hist = want_hist
    assert B == 1 or size == (1, 1) or (holes > 0 and filled > 0)
    assert B > 1 or holes == 0


def test_device_refusals(pkg, ctx):
    import torch
    W, H, B = 7, 5, 2
    n = W * H
    buf = torch.zeros(4096 + 400 * n, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 16 == 0
    d_hits, d_alb, d_motion, d_hist, d_hout, d_rgbz, d_rgbt, d_owner, d_hole, d_rays, d_keys = (
        base + 16 * i for i in (0, 3 * n, 4 * n, 4 * n + 18, 8 * n + 18, 12 * n + 18, 13 * n + 18, 14 * n + 18, 15 * n + 18, 16 * n + 18, 18 * n + 18))
    prev, cur = lens_camera(pkg, W, H, 4), lens_camera(pkg, W, H, 4)
    td, sd = pkg.temporal_desc(W, H), pkg.sparse_desc(W, H, block=B)
    ref = lambda d: ctypes.byref(d) if d is not None else None

    def rays(s=sd, f=cur, a=None, c=ctx._h):
        return pkg.hip.rtu_sparse_rays_device(c, ref(s), ref(f), *(a or [d_rays, d_keys, d_owner]), None)

    def acc(t=td, s=sd, p=prev, c=cur, a=None, cap=0):
        a = a or [d_rgbt, d_owner, d_hits, d_alb, d_hist, d_hout, d_rgbz, d_hole, d_motion]
        return pkg.hip.rtu_temporal_accumulate_sparse_device(ctx._h, ref(t), ref(s), ref(p), ref(c), *a, 3, cap, None)

    def fill(t=td, s=sd, a=None):
        return pkg.hip.rtu_sparse_fill_device(ctx._h, ref(t), ref(s), *(a or [d_hits, d_alb, d_owner, d_rgbt, d_hole, d_rgbz]), None)

    assert rays() == acc() == fill() == pkg.RTU_OK
    assert acc(a=[d_rgbt, d_owner, d_hits, d_alb, d_hist, d_hout, d_rgbz, d_hole + 1, d_motion]) == pkg.RTU_OK  # the hole plane: any alignment
    assert fill(a=[d_hits, d_alb, d_owner, d_rgbt, d_hole + 3, d_rgbz]) == pkg.RTU_OK
    bad_descs = [pkg.sparse_desc(W, H, block=0), pkg.sparse_desc(W, H, block=5), pkg.sparse_desc(W + 1, H, block=B), pkg.sparse_desc(0, 0, block=B), None]
    r = pkg.sparse_desc(W, H, block=B)
    r.reserved[2] = 1
    for s in bad_descs + [r]:
        assert rays(s=s) == acc(s=s) == fill(s=s) == pkg.RTU_ERR_ARG
    full = [d_rays, d_keys, d_owner]
    for i in range(3):
        assert rays(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
        assert rays(a=[p + 2 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG
    assert rays(a=[d_rays + 8, d_keys, d_owner]) == rays(f=None) == rays(f=lens_camera(pkg, W + 1, H, 4)) == rays(f=lens_camera(pkg, W, H, 0)) == pkg.RTU_ERR_ARG
    assert rays(c=None) == pkg.RTU_ERR_ARG
    full = [d_rgbt, d_owner, d_hits, d_alb, d_hist, d_hout, d_rgbz, d_hole, d_motion]
    for i in (0, 1, 2, 3, 5, 6, 7, 8):
        assert acc(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    for i in (0, 2, 3, 4, 5, 6, 8):  # float4 buffers and the table: 16-byte aligned
        assert acc(a=[p + 4 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    assert acc(a=[d_rgbt, d_owner + 2] + full[2:]) == pkg.RTU_ERR_ARG
    assert acc(a=full[:5] + [d_hist + 16] + full[6:]) == pkg.RTU_ERR_ARG, "overlapping histories"
    assert acc(p=None) == pkg.RTU_ERR_ARG and acc(p=None, a=full[:4] + [None] + full[5:]) == pkg.RTU_OK
    assert acc(cap=-1) == acc(cap=65536) == acc(t=None) == acc(c=None) == acc(t=pkg.temporal_desc(W, H, max_history=0)) == pkg.RTU_ERR_ARG
    assert acc(t=pkg.temporal_desc(W, H + 1)) == acc(c=lens_camera(pkg, W, H + 1, 4)) == pkg.RTU_ERR_ARG
    full = [d_hits, d_alb, d_owner, d_rgbt, d_hole, d_rgbz]
    for i in range(6):
        assert fill(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    for i in (0, 1, 3, 5):
        assert fill(a=[p + 4 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    assert fill(a=[d_hits, d_alb, d_owner + 2, d_rgbt, d_hole, d_rgbz]) == pkg.RTU_ERR_ARG
    assert fill(t=None) == fill(t=pkg.temporal_desc(W, H, sigma_plane=0.0)) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()


# ---- 2. sessions against the hand-assembled form ------------------------------------------------------------------------------------
def hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, B, motion, cap):
    """Frame k by hand: the host owners and rays, the existing ray-batch shading, frame_features, then the host forms of the sparse
    accumulator, the fill, the variance and the filter -> (image, history, holes)."""
    H, W = frame.height, frame.width
    sd = pkg.sparse_desc(W, H, block=B, frame_index=k)
    rays, keys, owner = pkg.sparse_rays(frame, sd)
    shade = ctx.shade_rays_paths if frame.gather_bounces else ctx.shade_rays_sampled
    rgbt = shade(rays, keys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0]
    hits, albedo = ctx.frame_features(frame)
    out, hist, hole = pkg.temporal_accumulate_sparse(prev, frame, rgbt, owner, hits, albedo, motion, hist, desc, sd, cap)
    out = pkg.sparse_fill(out, hole, hits, albedo, owner, rgbt, desc, sd)
    v = pkg.variance(hist, hits, vdesc)
    return pkg.denoise_variance(out, hits, albedo, v, vdesc), hist, int(hole.sum())


@pytest.mark.parametrize("tag,kw,distance,B,size", [("p10_s4_160x120", {"samples": 3}, 20.0, 2, None),
                                                    ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0, 2, None),
                                                    ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0, 3, (118, 67))], ids=["S-B2", "P-B2", "P-B3"])
def test_session_equals_the_hand_form(pkg, ctx, golden, tag, kw, distance, B, size):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = size or (g.width, g.height)
    assert B != 3 or (W % 3 and H % 3), "partial blocks in both axes"
    ctx.upload(scene)
    n_frames = 2 * B * B + 1 if B == 2 else B * B + 1
    frames = orbit_frames(pkg, scene, W, H, n_frames, distance, 0.25, **kw)
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    still = table("static", scene.desc.n_nodes)
    s = ctx.temporal(desc, variance=pkg.variance_desc(), sparse=pkg.sparse_desc(block=B))
    try:
        assert s.holes() == 0 and not s.history().any()
        prev = hist = None
        counts = []
        for k, frame in enumerate(frames):
            got = s.frame(frame)
            want, hist, holes = hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, B, still, 0)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3])), "frame %d: history" % k
            assert s.holes() == holes, "frame %d: holes" % k
            counts.append(holes)
        print("%s B %d: holes per frame %s of %d pixels" % (tag, B, counts, W * H))
        assert counts[0] == W * H - grid(W, H, B)[0] * grid(W, H, B)[1], "frame 0: every pixel but the owners is a hole"
        assert counts[-1] < counts[0], "the history filled no hole"
    finally:
        s.close()


def test_moved_session_equals_the_hand_form(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    W, H, B = g.width, g.height, 2
    scenes = animated(pkg, g.scene(pkg), 4, 20.0, 0.2)
    frames = [pkg.frame_setup(sc.desc.camera, W, H, samples=3) for sc in scenes]
    ctx.upload(scenes[0])
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    s = ctx.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(W, H, block=B))
    try:
        prev = hist = None
        for k, frame in enumerate(frames):
            if k:
                ctx.update(scenes[k])  # rtu_update_scene
            motion = pkg.scene_motion(scenes[k - 1] if k else scenes[0], scenes[k])
            want, hist, holes = hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, B, motion, 3)
            got = s.frame_moved(frame, motion, 3)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3])) and s.holes() == holes
        assert (hist[0][..., 3] >= 2).any(), "no history was carried across the updates"
    finally:
        s.close()


# ---- 3. the contract ---------------------------------------------------------------------------------------------------------------
def test_session_contract(pkg, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    frames = orbit_frames(pkg, scene, W, H, 4, 20.0, 0.5, samples=4)
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc()
    c = pkg.Context(0)
    try:
        a = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2))
        with pytest.raises(pkg.RtuError) as e:      # before an upload
            a.frame(frames[0])
        assert e.value.code == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        # a variance session on the same context keeps its bits, before and after; block == 1 is a variance session
        before = c.temporal(desc, variance=vdesc)
        ref = [before.frame(f) for f in frames]
        before.close()
        one = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=1))
        for f, r in zip(frames, ref):
            assert np.array_equal(bits(one.frame(f)), bits(r)) and one.holes() == 0
        one.close()
        render0 = c.render(frames[1])[0]
        differs = 0
        for k, f in enumerate(frames):
            a0 = pkg.hip.rtu_debug_device_allocations()
            got = a.frame(f)
            assert k == 0 or pkg.hip.rtu_debug_device_allocations() == a0, "frame %d of a sparse session allocated" % k
            differs += int((bits(got) != bits(ref[k])).sum())
            if k == 1:  # a render between two frames is unchanged and has no effect (the next frames equal the twin's below)
                assert np.array_equal(bits(c.render(frames[1])[0]), bits(render0))
        assert differs > 0
        twin = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(W, H, block=2))
        last = [twin.frame(f) for f in frames][-1]
        assert np.array_equal(bits(last), bits(got)) and twin.holes() == a.holes(), "a render between two frames changed the session"
        twin.close()
        after = c.temporal(desc, variance=vdesc)
        for f, r in zip(frames, ref):
            assert np.array_equal(bits(after.frame(f)), bits(r)), "a variance session lost its bits beside a sparse one"
        with pytest.raises(pkg.RtuError):
            after.holes()  # not a sparse session
        after.close()
        # reset, and a plain frame after an update, start over
        a.reset()
        assert a.holes() == 0 and not a.history().any()
        first = a.frame(frames[0])
        h0 = a.holes()
        assert a.history().max() == 1 and h0 > W * H // 2
        a.frame(frames[1])
        assert a.holes() < h0  # another pixel of every block
        c.update(scene)
        again = a.frame(frames[0])
        assert a.history().max() == 1 and a.holes() == h0 and np.array_equal(bits(again), bits(first)), "a plain frame after an update starts over"
        # the refusals
        for over in ({"block": 0}, {"block": 5}, {"block": -1}, {"width": W + 1, "height": H}, {"width": W, "height": 0}):
            with pytest.raises(pkg.RtuError) as e:
                c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(**over))
            assert e.value.code == pkg.RTU_ERR_ARG, over
        bd = pkg.sparse_desc()
        bd.reserved[3] = 1
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=vdesc, sparse=bd)
        with pytest.raises(pkg.RtuError):
            c.temporal(pkg.temporal_desc(W, H, denoise=True), variance=vdesc, sparse=pkg.sparse_desc())
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=pkg.variance_desc(n_passes=0), sparse=pkg.sparse_desc())
        for kw in ({"steer": pkg.steer_desc(budget=16)}, {"gradient": pkg.gradient_desc()}):  # out of scope: no such session
            with pytest.raises(pkg.RtuError):
                c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(), **kw)
        err, sd = ctypes.c_int(0), pkg.sparse_desc()
        begin = pkg.hip.rtu_temporal_begin_sparse
        assert not begin(None, ctypes.byref(desc), ctypes.byref(vdesc), ctypes.byref(sd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not begin(c._h, ctypes.byref(desc), ctypes.byref(vdesc), None, ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not begin(c._h, ctypes.byref(desc), None, ctypes.byref(sd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert not begin(c._h, None, ctypes.byref(vdesc), ctypes.byref(sd), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_holes(a._h, None) == pkg.RTU_ERR_ARG and pkg.hip.rtu_temporal_holes(None, ctypes.byref(ctypes.c_uint32())) == pkg.RTU_ERR_ARG
        # free after rtu_destroy_context: the handle stays valid for that alone
        held = pkg.hip.rtu_debug_device_bytes()
        c.close()
        assert pkg.hip.rtu_debug_device_bytes() < held - 232 * W * H + 1, "the session's buffers outlived the context"
        assert pkg.hip.rtu_temporal_holes(a._h, ctypes.byref(ctypes.c_uint32())) == pkg.RTU_ERR_ARG
        a.close()
    finally:
        c.close()
