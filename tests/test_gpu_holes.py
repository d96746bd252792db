"""GPU: hole rays (include/rtu_render.h "Hole rays"). The two device forms (rtu_hole_allocation_device, rtu_hole_fold_device) against
their host forms (which tests/test_holes_host.py holds to the rules), bit for bit; the frames of a sparse session with hole rays,
plain and moved, against the same steps assembled by hand from the host forms; the session's contract."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES
from test_gpu_ray_query import bits
from test_gpu_sparse import PAD, padded
from test_gpu_temporal import dev, orbit_frames
from test_gpu_temporal_motion import animated
from test_gpu_variance import ctx, fresh, same_bytes  # noqa: F401 (ctx: a fixture)
from test_holes_host import BUDGET_MAX, fold_samples, hole_planes, valid_of
from test_sparse_host import grid
from test_temporal_host import clone
from test_temporal_motion_host import table

pytestmark = pytest.mark.gpu

F = np.float32
U = np.uint32
GPU_SIZES = SIZES + [(200, 150)]  # more than one workgroup, a last tile that is not full, a last lane with fewer than four pixels (67 x 35)
SCAN_SIZE = (640, 410)            # 257 scan tiles: more than one tile per lane in k_steer_sums


def at_odd_offset(a, off):
    """`a` on the device `off` bytes into a buffer, PAD guard bytes behind it: (the buffer, the address of the bytes)."""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    d = fresh(off + len(raw) + PAD)
    d[off:off + len(raw)].copy_(torch.from_numpy(raw.copy()))
    return d, d.data_ptr() + off


def check_out(d, want, what, off=0):
    g = d.cpu().numpy()
    wb = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
    bad = g[off:off + len(wb)] != wb
    assert not bad.any(), "%s: %d bytes differ, first at %d" % (what, bad.sum(), np.flatnonzero(bad)[0])
    assert (g[:off] == 0x5A).all() and (g[off + len(wb):] == 0x5A).all(), "%s: written outside the array" % what


# ---- 1. the device forms against the host forms --------------------------------------------------------------------------------------
@pytest.mark.parametrize("size,B", [(s, 2) for s in GPU_SIZES] + [((67, 35), 4), ((200, 150), 3), (SCAN_SIZE, 2)], ids=lambda v: str(v).replace(" ", ""))
def test_allocation_device_equals_the_host_form(pkg, ctx, size, B):
    import torch
    W, H = size
    n = W * H
    stream = torch.cuda.Stream(device=0)
    taken = i = 0
    for hole, hits, _, _, _ in hole_planes(pkg, W, H, B, 2):
        wsum = int(((hole == 1) & valid_of(hits, H, W)).sum())
        d_hits = dev(hits)
        for budget in sorted({0, 1, wsum // 2, max(wsum - 1, 0), wsum, BUDGET_MAX}):
            for k in (0, 0xffffffff):
                desc = pkg.hole_desc(W, H, budget=budget, frame_index=k)
                counts, offsets, total = pkg.hole_allocation(hole, hits, desc)
                off = i % 4  # the hole plane at every alignment
                d_hole, hole_ptr = at_odd_offset(hole, off)
                d_counts, d_offsets, d_total = fresh(4 * n + PAD), fresh(4 * n + PAD), fresh(4 + PAD)
                s = stream if i % 2 else None
                if i == 0:  # (the first call at a size may grow the context's scratch)
                    ctx.hole_allocation_device(desc, hole_ptr, d_hits.data_ptr(), d_counts.data_ptr(), d_offsets.data_ptr(), d_total.data_ptr(), None)
                torch.cuda.synchronize()
                a0 = pkg.hip.rtu_debug_device_allocations()
                ctx.hole_allocation_device(desc, hole_ptr, d_hits.data_ptr(), d_counts.data_ptr(), d_offsets.data_ptr(), d_total.data_ptr(),
                                           s.cuda_stream if s else None)
                (s or torch.cuda).synchronize()
                assert pkg.hip.rtu_debug_device_allocations() == a0, "a second call at a size allocated"
                where = "budget %d frame %d offset %d" % (budget, k, off)
                check_out(d_counts, counts, "counts, " + where)
                check_out(d_offsets, offsets, "offsets, " + where)
                check_out(d_total, np.array([total], U), "total, " + where)
                check_out(d_hole, hole, "the hole plane was written, " + where, off)
                assert same_bytes(d_hits, hits), "an input was written"
                taken += total
                i += 1
    assert size == (1, 1) or taken > 0


@pytest.mark.parametrize("size,B", [(s, 2) for s in GPU_SIZES] + [((67, 35), 4), ((200, 150), 3)], ids=lambda v: str(v).replace(" ", ""))
def test_fold_device_equals_the_host_form(pkg, ctx, size, B):
    import torch
    W, H = size
    n = W * H
    stream = torch.cuda.Stream(device=0)
    folded = i = 0
    desc = pkg.hole_desc(W, H)
    for k, (hole, hits, hist, out, albedo) in enumerate(hole_planes(pkg, W, H, B, 2)):
        wsum = int(((hole == 1) & valid_of(hits, H, W)).sum())
        d_hits, d_alb = dev(hits), dev(albedo)
        for budget in (BUDGET_MAX, (2 * wsum) // 3):
            counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=budget, frame_index=k))
            rgbt = fold_samples(total, 7 * k + B)
            want_out, want_hist, want_hole = pkg.hole_fold(hist, out, hole, hits, albedo, counts, offsets, rgbt)
            off = (i + 1) % 4
            d_hist, d_out = padded(hist), padded(out)
            d_hole, hole_ptr = at_odd_offset(hole, off)
            d_counts, d_offsets, d_rgbt = dev(counts), dev(offsets), dev(rgbt) if total else fresh(16)
            s = stream if i % 2 else None
            torch.cuda.synchronize()
            a0 = pkg.hip.rtu_debug_device_allocations()
            ctx.hole_fold_device(desc, d_hist.data_ptr(), d_out.data_ptr(), hole_ptr, d_hits.data_ptr(), d_alb.data_ptr(), d_counts.data_ptr(),
                                 d_offsets.data_ptr(), d_rgbt.data_ptr(), total, s.cuda_stream if s else None)
            (s or torch.cuda).synchronize()
            assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
            check_out(d_hist, want_hist, "history, frame %d budget %d" % (k, budget))
            check_out(d_out, want_out, "image, frame %d budget %d" % (k, budget))
            check_out(d_hole, want_hole, "hole plane, frame %d budget %d" % (k, budget), off)
            assert same_bytes(d_hits, hits) and same_bytes(d_alb, albedo) and same_bytes(d_counts, counts) and same_bytes(d_offsets, offsets), "an input was written"
            assert not total or same_bytes(d_rgbt, rgbt), "an input was written"
            folded += int((want_hole != hole).sum())
            i += 1
    assert size == (1, 1) or folded > 0


def test_fold_device_with_adversarial_counts_and_offsets(pkg, ctx):
    """A count of 7 is one sample; an offset at or beyond n_rays is not read and its pixel not written: the device form gives what the
    host form gives for the counts and offsets with those entries made harmless."""
    import torch
    W, H, B = 67, 35, 2
    hole, hits, hist, out, albedo = hole_planes(pkg, W, H, B, 1)[0]
    counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=BUDGET_MAX))
    assert total > 40
    rgbt = fold_samples(total, 3)
    picked = np.flatnonzero(counts.reshape(-1))
    bad_counts, bad_offsets = counts.copy().reshape(-1), offsets.copy().reshape(-1)
    bad_counts[picked[0::5]] = 7
    bad_counts[picked[1::5]] = 0xffffffff
    bad_offsets[picked[2::5]] = total
    bad_offsets[picked[3::5]] = 0xffffffff
    bad_offsets[picked[4::10]] = total + 1
    safe_counts, safe_offsets = np.minimum(bad_counts, 1), bad_offsets.copy()
    beyond = bad_offsets >= total
    safe_counts[beyond] = 0
    safe_offsets[beyond] = 0
    want_out, want_hist, want_hole = pkg.hole_fold(hist, out, hole, hits, albedo, safe_counts, safe_offsets, rgbt)
    assert (want_hole.reshape(-1)[picked[2::5]] == 1).all() and (want_hole != hole).any()
    d_hist, d_out, d_hole, d_rgbt = padded(hist), padded(out), padded(hole), padded(rgbt)
    d_hits, d_alb, d_counts, d_offsets = dev(hits), dev(albedo), dev(bad_counts), dev(bad_offsets)
    ctx.hole_fold_device(pkg.hole_desc(W, H), d_hist.data_ptr(), d_out.data_ptr(), d_hole.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                         d_counts.data_ptr(), d_offsets.data_ptr(), d_rgbt.data_ptr(), total, None)
    torch.cuda.synchronize()
    check_out(d_hist, want_hist, "history")
    check_out(d_out, want_out, "image")
    check_out(d_hole, want_hole, "hole plane")
    check_out(d_rgbt, rgbt, "the samples were written")


def test_device_refusals(pkg, ctx):
    import torch
    W, H = 7, 5
    n = W * H
    buf = torch.zeros(4096 + 200 * n, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    assert base % 16 == 0
    d_hits, d_alb, d_hist, d_rgbz, d_rgbt, d_counts, d_offsets, d_total, d_hole = (base + 16 * i for i in (0, 3 * n, 4 * n, 8 * n, 9 * n, 10 * n, 11 * n, 12 * n, 12 * n + 1))
    hd = pkg.hole_desc(W, H, budget=n)
    ref = lambda d: ctypes.byref(d) if d is not None else None

    def alloc(d=hd, a=None, c=ctx._h):
        return pkg.hip.rtu_hole_allocation_device(c, ref(d), *(a or [d_hole, d_hits, d_counts, d_offsets, d_total]), None)

    def fold(d=hd, a=None, n_rays=0, c=ctx._h):
        a = a or [d_hist, d_rgbz, d_hole, d_hits, d_alb, d_counts, d_offsets, d_rgbt]
        return pkg.hip.rtu_hole_fold_device(c, ref(d), *a, n_rays, None)

    assert alloc() == fold() == fold(n_rays=n) == pkg.RTU_OK
    for off in (1, 2, 3):  # the hole plane: any alignment
        assert alloc(a=[d_hole + off, d_hits, d_counts, d_offsets, d_total]) == pkg.RTU_OK
        assert fold(a=[d_hist, d_rgbz, d_hole + off, d_hits, d_alb, d_counts, d_offsets, d_rgbt], n_rays=n) == pkg.RTU_OK
    r = pkg.hole_desc(W, H)
    r.reserved[1] = 1
    for d in (None, pkg.hole_desc(0, 0), pkg.hole_desc(W, 0), pkg.hole_desc(65537, 1), pkg.hole_desc(W, H, budget=BUDGET_MAX + 1), r):
        assert alloc(d=d) == fold(d=d) == pkg.RTU_ERR_ARG
    assert alloc(c=None) == fold(c=None) == pkg.RTU_ERR_ARG
    full = [d_hole, d_hits, d_counts, d_offsets, d_total]
    for i in range(5):
        assert alloc(a=[None if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    for i in (1, 2, 3, 4):
        assert alloc(a=[p + 2 if j == i else p for j, p in enumerate(full)]) == pkg.RTU_ERR_ARG, i
    assert alloc(a=[d_hole, d_hits + 4, d_counts, d_offsets, d_total]) == pkg.RTU_ERR_ARG
    full = [d_hist, d_rgbz, d_hole, d_hits, d_alb, d_counts, d_offsets, d_rgbt]
    for i in range(8):
        assert fold(a=[None if j == i else p for j, p in enumerate(full)], n_rays=n) == pkg.RTU_ERR_ARG, i
    assert fold(a=full[:7] + [None]) == pkg.RTU_OK  # no rays: no samples
    for i in (0, 1, 3, 4, 7):  # float4 buffers: 16-byte aligned
        assert fold(a=[p + 4 if j == i else p for j, p in enumerate(full)], n_rays=n) == pkg.RTU_ERR_ARG, i
    for i in (5, 6):
        assert fold(a=[p + 2 if j == i else p for j, p in enumerate(full)], n_rays=n) == pkg.RTU_ERR_ARG, i
    assert fold(n_rays=BUDGET_MAX + 1) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()


# ---- 2. sessions against the hand-assembled form ------------------------------------------------------------------------------------
def hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, B, budget, motion, cap):
    """Frame k by hand: the host owners and rays, the existing ray-batch shading, frame_features, the host sparse accumulator, the host
    allocation, rtu_extra_sample_rays, the shading again, the host fold, then the host fill, variance and filter -> (image, history,
    holes, hole rays)."""
    H, W = frame.height, frame.width
    sd = pkg.sparse_desc(W, H, block=B, frame_index=k)
    shade = ctx.shade_rays_paths if frame.gather_bounces else ctx.shade_rays_sampled
    rays, keys, owner = pkg.sparse_rays(frame, sd)
    rgbt = shade(rays, keys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0]
    hits, albedo = ctx.frame_features(frame)
    out, hist, hole = pkg.temporal_accumulate_sparse(prev, frame, rgbt, owner, hits, albedo, motion, hist, desc, sd, cap)
    counts, offsets, total = pkg.hole_allocation(hole, hits, pkg.hole_desc(budget=budget, frame_index=k))
    if total:
        hrays, hkeys, howner = pkg.extra_sample_rays(frame, counts, offsets, pkg.steer_desc(budget=budget, max_extra=1, frame_index=k))
        assert len(hrays) == total and np.array_equal(howner, np.flatnonzero(counts.reshape(-1)))
        samples = shade(hrays, hkeys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0]
        out, hist, hole = pkg.hole_fold(hist, out, hole, hits, albedo, counts, offsets, samples)
    out = pkg.sparse_fill(out, hole, hits, albedo, owner, rgbt, desc, sd)
    v = pkg.variance(hist, hits, vdesc)
    return pkg.denoise_variance(out, hits, albedo, v, vdesc), hist, int(hole.sum()), total


SESSIONS = [("p10_s4_160x120", {"samples": 3}, 20.0, 2, None), ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0, 2, None),
            ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0, 3, (118, 67))]


@pytest.mark.parametrize("budget", [BUDGET_MAX, 100], ids=["full", "100"])
@pytest.mark.parametrize("tag,kw,distance,B,size", SESSIONS, ids=["S-B2", "P-B2", "P-B3"])
def test_session_equals_the_hand_form(pkg, ctx, golden, tag, kw, distance, B, size, budget):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = size or (g.width, g.height)
    ctx.upload(scene)
    n_frames = 2 * B * B + 1
    frames = orbit_frames(pkg, scene, W, H, n_frames, distance, 0.25, **kw)
    frames[-2] = frames[-3]  # one frame at rest: with the full budget it has no hole ray
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    still = table("static", scene.desc.n_nodes)
    s = ctx.temporal(desc, variance=pkg.variance_desc(), sparse=pkg.sparse_desc(block=B), holes=pkg.hole_desc(budget=budget))
    try:
        assert s.holes() == 0 and s.hole_rays() == 0 and not s.history().any()
        prev = hist = None
        holes, rays = [], []
        for k, frame in enumerate(frames):
            got = s.frame(frame)
            want, hist, n_holes, n_rays = hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, B, budget, still, 0)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3])), "frame %d: history" % k
            assert s.holes() == n_holes and s.hole_rays() == n_rays, "frame %d: holes %d (%d), hole rays %d (%d)" % (k, s.holes(), n_holes, s.hole_rays(), n_rays)
            holes.append(n_holes)
            rays.append(n_rays)
        print("%s B %d budget %d: hole rays per frame %s, holes filled %s of %d pixels" % (tag, B, budget, rays, holes, W * H))
        assert max(rays) <= budget and rays[0] > 0
        if budget == BUDGET_MAX:
            blocks = grid(W, H, B)[0] * grid(W, H, B)[1]
            assert rays[0] + holes[0] == W * H - blocks, "frame 0: every pixel but the owners is shaded or, a miss, filled"
            assert rays[-2] == 0, "at rest every VALID pixel has its history"
        else:
            assert holes[0] > holes[-1], "the dither takes about 100 of the holes of frame 0, the history and later rays fill the rest"
    finally:
        s.close()


def test_moved_session_equals_the_hand_form(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    W, H, B = g.width, g.height, 2
    scenes = animated(pkg, g.scene(pkg), 4, 20.0, 0.2)
    frames = [pkg.frame_setup(sc.desc.camera, W, H, samples=3) for sc in scenes]
    ctx.upload(scenes[0])
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc(W, H)
    s = ctx.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(W, H, block=B), holes=pkg.hole_desc(W, H, budget=BUDGET_MAX))
    try:
        prev = hist = None
        rays = []
        for k, frame in enumerate(frames):
            if k:
                ctx.update(scenes[k])  # rtu_update_scene
            motion = pkg.scene_motion(scenes[k - 1] if k else scenes[0], scenes[k])
            want, hist, n_holes, n_rays = hand_frame(pkg, ctx, frame, k, prev, hist, desc, vdesc, B, BUDGET_MAX, motion, 3)
            got = s.frame_moved(frame, motion, 3)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3])) and s.holes() == n_holes and s.hole_rays() == n_rays
            rays.append(n_rays)
        print("moved: hole rays per frame %s" % rays)
        assert rays[0] > 0 and sum(rays[1:]) > 0, "no hole ray after an update: %s" % rays
        assert (hist[0][..., 3] >= 2).any(), "no history was carried across the updates"
    finally:
        s.close()


# ---- 3. the contract ---------------------------------------------------------------------------------------------------------------
def test_session_contract(pkg, golden):
    g = golden("p11_p2_120x68")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    kw = {"samples": 4, "gather_bounces": 4}
    frames = orbit_frames(pkg, scene, W, H, 4, 60.0, 0.5, **kw)
    away = clone(pkg, scene)  # the camera turned round: every ray misses
    away.desc.camera.dir[:] = [-float(x) for x in scene.desc.camera.dir]
    nothing = pkg.frame_setup(away.desc.camera, W, H, **kw)
    desc, vdesc = pkg.temporal_desc(W, H), pkg.variance_desc()
    full = lambda: pkg.hole_desc(budget=BUDGET_MAX)
    c = pkg.Context(0)
    try:
        a = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2), holes=full())
        with pytest.raises(pkg.RtuError) as e:      # before an upload
            a.frame(frames[0])
        assert e.value.code == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        # a sparse session on the same context keeps its bits, before and after; budget 0 is a sparse session, block 1 a variance session
        before = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2))
        ref = [(before.frame(f), before.holes()) for f in frames + [nothing]]
        before.close()
        plain = c.temporal(desc, variance=vdesc)
        ref1 = [plain.frame(f) for f in frames]
        plain.close()
        zero = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2), holes=pkg.hole_desc(W, H, budget=0))
        for f, (r, h) in zip(frames + [nothing], ref):
            assert np.array_equal(bits(zero.frame(f)), bits(r)) and zero.holes() == h and zero.hole_rays() == 0, "budget 0 is not the sparse session"
        zero.close()
        one = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=1), holes=full())
        for f, r in zip(frames, ref1):
            assert np.array_equal(bits(one.frame(f)), bits(r)) and one.holes() == 0 and one.hole_rays() == 0, "block 1 is not the variance session"
        one.close()
        # a frame with total 0 — nothing but misses — equals the budget-0 frame and launches no second batch
        only = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2), holes=full())
        lone = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2))
        for _ in range(2):
            got, want = only.frame(nothing), lone.frame(nothing)
            assert np.array_equal(bits(got), bits(want)) and only.hole_rays() == 0 and only.holes() == lone.holes() > 0
        only.close()
        lone.close()
        render0 = c.render(frames[1])[0]
        differs, rays = 0, []
        for k, f in enumerate(frames):
            got = a.frame(f)
            differs += int((bits(got) != bits(ref[k][0])).sum())
            rays.append(a.hole_rays())
            assert a.holes() <= ref[k][1], "frame %d: more holes to fill than the sparse session had" % k
            if k == 1:  # a render between two frames is unchanged and has no effect (the next frames equal the twin's below)
                assert np.array_equal(bits(c.render(frames[1])[0]), bits(render0))
        assert differs > 0 and rays[0] > 0 and (a.history() >= 1).sum() > W * H // 2
        twin = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(W, H, block=2), holes=pkg.hole_desc(W, H, budget=BUDGET_MAX))
        last = [twin.frame(f) for f in frames][-1]
        assert np.array_equal(bits(last), bits(got)) and twin.holes() == a.holes() and twin.hole_rays() == a.hole_rays(), \
            "a render between two frames changed the session"
        # at rest every VALID pixel has its history: no hole ray, and nothing is allocated
        a0 = pkg.hip.rtu_debug_device_allocations()
        twin.frame(frames[-1])
        assert twin.hole_rays() == 0 and pkg.hip.rtu_debug_device_allocations() == a0
        twin.close()
        after = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2))
        for f, (r, h) in zip(frames + [nothing], ref):
            assert np.array_equal(bits(after.frame(f)), bits(r)) and after.holes() == h, "a sparse session lost its bits beside one with hole rays"
        with pytest.raises(pkg.RtuError):
            after.hole_rays()  # not a session with hole rays
        after.close()
        # reset, and a plain frame after an update, start over
        a.reset()
        assert a.holes() == 0 and a.hole_rays() == 0 and not a.history().any()
        first = a.frame(frames[0])
        h0, r0 = a.holes(), a.hole_rays()
        assert a.history().max() == 1 and r0 == rays[0] and r0 + h0 == W * H - (W // 2) * (H // 2)
        a.frame(frames[1])
        assert a.hole_rays() < r0
        c.update(scene)
        again = a.frame(frames[0])
        assert a.history().max() == 1 and a.holes() == h0 and a.hole_rays() == r0 and np.array_equal(bits(again), bits(first)), \
            "a plain frame after an update starts over"
        # the 2 S refusal leaves the session as it was: the next frame is the twin's
        a.frame(frames[1])
        many = pkg.frame_setup(scene.desc.camera, W, H, samples=32769, gather_bounces=4)
        with pytest.raises(pkg.RtuError) as e:
            a.frame(many)
        assert e.value.code == pkg.RTU_ERR_ARG and "hole rays" in str(e.value)
        twin = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2), holes=full())
        want = [twin.frame(f) for f in frames[:3]][-1]
        assert np.array_equal(bits(a.frame(frames[2])), bits(want)) and a.hole_rays() == twin.hole_rays(), "a refused frame moved the frame counter"
        twin.close()
        zero = c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=2), holes=pkg.hole_desc(budget=0))
        zero.frame(many)  # without hole rays 2 S is no limit of the frame
        zero.close()
        # the refusals at begin
        for over in ({"budget": BUDGET_MAX + 1}, {"width": W + 1, "height": H}, {"width": W, "height": 0}, {"width": 0, "height": H}):
            with pytest.raises(pkg.RtuError) as e:
                c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(), holes=pkg.hole_desc(**over))
            assert e.value.code == pkg.RTU_ERR_ARG, over
        for i in range(4):
            bd = pkg.hole_desc()
            bd.reserved[i] = 1
            with pytest.raises(pkg.RtuError):
                c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(), holes=bd)
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=vdesc, sparse=pkg.sparse_desc(block=5), holes=full())  # what a sparse session refuses
        with pytest.raises(pkg.RtuError):
            c.temporal(desc, variance=vdesc, holes=full())  # hole rays belong to a sparse session
        err, sd, hd = ctypes.c_int(0), pkg.sparse_desc(), full()
        begin = pkg.hip.rtu_temporal_begin_sparse_holes
        args = [ctypes.byref(desc), ctypes.byref(vdesc), ctypes.byref(sd), ctypes.byref(hd)]
        assert not begin(None, *args, ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        for i in range(4):
            assert not begin(c._h, *[None if j == i else p for j, p in enumerate(args)], ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG, i
        assert pkg.hip.rtu_temporal_hole_rays(a._h, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_hole_rays(None, ctypes.byref(ctypes.c_uint32())) == pkg.RTU_ERR_ARG
        # free after rtu_destroy_context: the handle stays valid for that alone
        held = pkg.hip.rtu_debug_device_bytes()
        c.close()
        assert pkg.hip.rtu_debug_device_bytes() < held - (232 + 12) * W * H + 1, "the session's buffers outlived the context"
        assert pkg.hip.rtu_temporal_hole_rays(a._h, ctypes.byref(ctypes.c_uint32())) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_holes(a._h, ctypes.byref(ctypes.c_uint32())) == pkg.RTU_ERR_ARG
        a.close()
    finally:
        c.close()
