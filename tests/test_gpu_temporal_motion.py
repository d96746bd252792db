"""GPU: temporal accumulation across scene updates (include/rtu_render.h "Temporal accumulation across scene updates"). The device
accumulator (rtu_temporal_accumulate_motion_device, k_temporal<true, false>) and the device motion vectors against their host forms (which
tests/test_temporal_motion_host.py holds to the rules), bit for bit; a session's moved frames against the same thing assembled by hand
from existing entries on the updated context; the session's contract."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES
from test_gpu_ray_query import bits
from test_gpu_temporal import dev, orbit_frames
from test_mesh_update_host import clone, deformed_scene
from test_temporal_host import FRAMES, chain_inputs, orbit_scene
from test_temporal_motion_host import CASES, STATIC, RESET, case_cameras, host_motion_form, run_motion_chain, table

pytestmark = pytest.mark.gpu

F = np.float32
MESH_NODE, SPHERE_NODE = 7, 8  # in both golden scenes used here: the teapot (mesh 0) and a sphere


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ---- 1. the device accumulator against the host form -------------------------------------------------------------------------------
def device_motion_form(pkg, ctx, streams, in_place_at):
    import torch
    state = {"k": 0, "hist": None}

    def form(prev, cur, rgbz, hits, albedo, hist, desc, motion, cap):
        H, W = rgbz.shape[:2]
        k = state["k"] = 0 if hist is None else state["k"] + 1
        d_in, d_hits, d_alb = dev(rgbz), dev(hits), dev(albedo)
        # (an empty table still needs a pointer: one entry that n_nodes == 0 keeps unread)
        d_motion = dev(motion) if len(motion) else torch.full((96,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d_prev = state["hist"] if hist is not None else None
        d_hist = torch.full((3 * H * W * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        in_place = k == in_place_at
        d_out = d_in if in_place else torch.full((H * W * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        s = streams[k % 2]
        table_before = d_motion.cpu().numpy()
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.temporal_accumulate_motion_device(desc, prev, cur, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                              d_prev.data_ptr() if d_prev is not None else None, d_hist.data_ptr(), d_out.data_ptr(),
                                              d_motion.data_ptr(), len(motion), cap, s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        if not in_place:
            assert np.array_equal(d_in.cpu().numpy(), np.ascontiguousarray(rgbz).view(np.uint8).reshape(-1)), "the input was written"
        assert np.array_equal(d_hits.cpu().numpy(), np.ascontiguousarray(hits).view(np.uint8).reshape(-1)), "the hits were written"
        assert np.array_equal(d_alb.cpu().numpy(), np.ascontiguousarray(albedo).view(np.uint8).reshape(-1)), "the albedo was written"
        assert np.array_equal(d_motion.cpu().numpy(), table_before), "the table was written"
        if d_prev is not None:
            assert np.array_equal(d_prev.cpu().numpy(), np.ascontiguousarray(hist).view(np.uint8).reshape(-1)), "the previous history was written"
        state["hist"] = d_hist
        return d_out.cpu().numpy().view(F).reshape(H, W, 4), d_hist.cpu().numpy().view(F).reshape(3, H, W, 4)
    return form


def compare_chain(pkg, ctx, stream, W, H, ci, case):
    kind, n, camname, cap, over = case
    cams = case_cameras(pkg, W, H, camname)
    frames = chain_inputs(pkg, W, H, 1234 + ci)
    desc = pkg.temporal_desc(W, H, **over)
    motion = table(kind)[:n]
    want = run_motion_chain(cams, frames, desc, motion, cap, host_motion_form(pkg))
    got = run_motion_chain(cams, frames, desc, motion, cap, device_motion_form(pkg, ctx, (None, stream), in_place_at=1 + ci % 4))
    for k in range(FRAMES):
        for what, g, w in (("image", got[k][0], want[k][0]), ("history", got[k][1], want[k][1])):
            diff = bits(g) != bits(w)
            assert not diff.any(), "table %s[%d] cameras %s cap %d %s frame %d %s: %d words differ, first at %s" % (
                kind, n, camname, cap, over, k, what, diff.sum(), np.argwhere(diff)[0])
    return want


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
def test_device_form_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    stream = torch.cuda.Stream(device=0)
    grown = False
    for ci, case in enumerate(CASES):
        want = compare_chain(pkg, ctx, stream, W, H, ci, case)
        grown |= bool((want[-1][1][0][..., 3] > 1).any())
    assert grown or size == (1, 1), "nothing was accumulated"


def test_device_form_equals_the_host_form_at_200x150(pkg, ctx):
    """More than one workgroup in both directions, neither a multiple of the 32 x 8 tile; the case that mixes one-tap and reprojecting
    lanes in one wavefront, and the one that normalises."""
    import torch
    stream = torch.cuda.Stream(device=0)
    for ci in (3, 5):
        compare_chain(pkg, ctx, stream, 200, 150, ci, CASES[ci])


def test_accumulate_motion_device_refusals(pkg, ctx):
    import torch
    from test_temporal_host import chain_cameras
    W, H = 7, 5
    n = W * H
    buf = torch.zeros(n * (16 + 48 + 16 + 48 + 48 + 16) + 3 * 96 + 64, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    ptrs = [base, base + 16 * n, base + 64 * n, base + 80 * n, base + 128 * n, base + 176 * n, base + 192 * n]  # ..., out, table
    buf[192 * n:192 * n + 3 * 96] = torch.from_numpy(table("slide").view(np.uint8).copy()).to("cuda:0")
    cams = chain_cameras(pkg, W, H)["X"]
    d = pkg.temporal_desc(W, H)

    def call(desc=d, p=ptrs, prev=cams[2], cur=cams[3], nn=3, cap=2):
        return pkg.hip.rtu_temporal_accumulate_motion_device(ctx._h, ctypes.byref(desc), ctypes.byref(prev) if prev is not None else None,
                                                             ctypes.byref(cur) if cur is not None else None, *p, nn, cap, None)
    assert call() == pkg.RTU_OK
    for k in range(7):
        p = list(ptrs)
        p[k] = None
        assert call(p=p, prev=None if k == 3 else cams[2]) == (pkg.RTU_OK if k == 3 else pkg.RTU_ERR_ARG), k  # hist_prev may be NULL, the table not
        p[k] = ptrs[k] + 8
        assert call(p=p) == pkg.RTU_ERR_ARG, k                                                                # misaligned, the table too
    p = list(ptrs)
    p[4] = ptrs[3]                      # aliased histories
    assert call(p=p) == pkg.RTU_ERR_ARG
    p[4] = ptrs[3] + 16                 # overlapping
    assert call(p=p) == pkg.RTU_ERR_ARG
    for cap in (-1, 65536):
        assert call(cap=cap) == pkg.RTU_ERR_ARG
    assert call(cap=0) == pkg.RTU_OK and call(cap=65535) == pkg.RTU_OK
    assert call(desc=pkg.temporal_desc(W, H, max_history=0)) == pkg.RTU_ERR_ARG and call(desc=pkg.temporal_desc(W + 1, H)) == pkg.RTU_ERR_ARG
    assert call(cur=None) == pkg.RTU_ERR_ARG and call(prev=None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_temporal_accumulate_motion_device(None, ctypes.byref(d), ctypes.byref(cams[2]), ctypes.byref(cams[3]), *ptrs, 3, 0, None) == pkg.RTU_ERR_ARG
    mv = lambda hits=ptrs[1], m=ptrs[6], out=ptrs[3], prev=cams[2]: pkg.hip.rtu_motion_vectors_device(
        ctx._h, ctypes.byref(d), ctypes.byref(prev) if prev is not None else None, hits, m, 3, out, None)
    assert mv() == pkg.RTU_OK
    assert mv(hits=None) == mv(m=None) == mv(out=None) == mv(prev=None) == mv(m=ptrs[6] + 4) == mv(out=ptrs[3] + 8) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()


# ---- 2. motion vectors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(67, 35), (200, 150)], ids=lambda s: "%dx%d" % s)
def test_motion_vectors_device_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    stream = torch.cuda.Stream(device=0)
    desc = pkg.temporal_desc(W, H)
    given = 0
    for ci, (kind, n, camname, cap, over) in enumerate(CASES):
        if size != (67, 35) and ci not in (2, 5, 8, 10):
            continue
        cams = case_cameras(pkg, W, H, camname)
        hits = chain_inputs(pkg, W, H, 1234 + ci)[1][1]
        motion = table(kind)[:n]
        want = pkg.motion_vectors(cams[0], hits, motion, W, H)
        d_hits = dev(hits)
        d_motion = dev(motion) if len(motion) else torch.full((96,), 0x5A, dtype=torch.uint8, device="cuda:0")
        d_mv = torch.full((H * W * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        s = stream if ci % 2 else None
        ctx.motion_vectors_device(desc, cams[0], d_hits.data_ptr(), d_motion.data_ptr(), len(motion), d_mv.data_ptr(), s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0
        got = d_mv.cpu().numpy().view(F).reshape(H, W, 4)
        diff = bits(got) != bits(want)
        assert not diff.any(), "table %s[%d] cameras %s: %d words differ, first at %s" % (kind, n, camname, diff.sum(), np.argwhere(diff)[0])
        given += int((want[..., 2] == 1).sum())
    assert given > 0


# ---- 3. sessions ----------------------------------------------------------------------------------------------------------------------
def animated(pkg, scene, n, distance, step):
    """n scenes: the mesh node and a sphere node moved a step further in each, and in the third also the camera."""
    out = []
    for k in range(n):
        s = clone(pkg, scene)
        s.node_translate(MESH_NODE, (step * k, 0.0, 0.0))
        s.node_translate(SPHERE_NODE, (0.0, 0.5 * step * k, 0.0))
        out.append(orbit_scene(pkg, s, 1, distance, 0.5) if k == 2 else s)
    return out


def hand_frame_moved(pkg, ctx, frame, k, prev, hist, desc, denoise, motion, cap):
    """Frame k by existing entries on the updated context: host rays -> host shading -> frame_features -> host motion accumulator
    (-> host filter)."""
    rays, keys = pkg.camera_sample_rays(frame, k % frame.samples)
    shade = ctx.shade_rays_paths if frame.gather_bounces else ctx.shade_rays_sampled
    rgbt = shade(rays, keys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0].reshape(frame.height, frame.width, 4)
    hits, albedo = ctx.frame_features(frame)
    out, hist = pkg.temporal_accumulate_motion(prev, frame, rgbt, hits, albedo, motion, hist, desc, cap)
    return (pkg.denoise(out, hits, albedo) if denoise else out), hist, hits


@pytest.mark.parametrize("tag,kw,distance,step", [("p10_s4_160x120", {"samples": 3}, 20.0, 0.2), ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0, 0.3)],
                         ids=["S", "P"])
@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoised"])
def test_moved_session_equals_the_hand_form(pkg, ctx, golden, tag, kw, distance, step, denoise):
    g = golden(tag)
    W, H = g.width, g.height
    scenes = animated(pkg, g.scene(pkg), 4, distance, step)
    frames = [pkg.frame_setup(s.desc.camera, W, H, **kw) for s in scenes]
    n_nodes = scenes[0].desc.n_nodes
    cap = 3 if denoise else 0
    ctx.upload(scenes[0])
    desc = pkg.temporal_desc(W, H, denoise=denoise)
    s = ctx.temporal(desc)
    try:
        prev = hist = None
        for k, frame in enumerate(frames):
            if k:
                ctx.update(scenes[k])
            motion = pkg.scene_motion(scenes[k - 1] if k else scenes[0], scenes[k])
            assert k == 0 or [i for i in range(n_nodes) if not motion["flags"][i] & STATIC] == [MESH_NODE, SPHERE_NODE]
            if k == 2:  # a wrong n_nodes is refused and changes nothing: the frames that follow still equal the hand form
                before = s.history()
                with pytest.raises(pkg.RtuError) as e:
                    s.frame_moved(frame, motion[:-1], cap)
                assert e.value.code == pkg.RTU_ERR_ARG
                assert pkg.hip.rtu_temporal_frame_moved(s._h, ctypes.byref(frame), None, n_nodes, cap, before.ctypes.data) == pkg.RTU_ERR_ARG
                assert pkg.hip.rtu_temporal_frame_moved(s._h, ctypes.byref(frame), motion.ctypes.data, n_nodes, -1, before.ctypes.data) == pkg.RTU_ERR_ARG
                bad = motion.copy()
                bad["reserved"][0][1] = 1
                with pytest.raises(pkg.RtuError):
                    s.frame_moved(frame, bad, cap)
                assert np.array_equal(bits(s.history()), bits(before))
            want, hist, hits = hand_frame_moved(pkg, ctx, frame, k, prev, hist, desc, denoise, motion, cap)
            a0 = pkg.hip.rtu_debug_device_allocations()
            got = s.frame_moved(frame, motion, cap)
            assert k == 0 or pkg.hip.rtu_debug_device_allocations() == a0, "moved frame %d allocated" % k
            motion[:] = 0  # the caller may reuse its table once the call returned
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3]))
        valid = ((hits["flags"] & 1) != 0).reshape(H, W)
        n = s.history()
        moved_px = valid & np.isin(hits["node"].reshape(H, W), (MESH_NODE, SPHERE_NODE))
        print("%s: history > 1 on %.1f %% of the valid pixels, on %.1f %% of the %d pixels of the moved nodes, max %.2f"
              % (tag, 100 * (n[valid] > 1).mean(), 100 * (n[moved_px] > 1).mean(), moved_px.sum(), n.max()))
        assert (n[valid] > 1).mean() > 0.5, "the updates left no history to speak of"
        assert moved_px.sum() > 100 and (n[moved_px] > 1).mean() > 0.5, "the moved nodes kept no history"
        # the existing behaviour, on the same session: a plain frame after an update starts over
        ctx.update(scenes[2])
        assert not s.history().any()
        s.frame(frames[2])
        n = s.history()
        assert set(np.unique(n)) <= {0.0, 1.0} and (n[valid] == 1).mean() > 0.9
    finally:
        s.close()


def test_static_table_equals_the_plain_session(pkg, ctx, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    frames = orbit_frames(pkg, scene, W, H, 3, 20.0, 0.5, samples=3)
    frames.append(frames[-1])  # the last camera at rest: the one-tap path
    motion = pkg.scene_motion(scene, scene)
    assert (motion["flags"] == STATIC).all()
    desc = pkg.temporal_desc(W, H)
    a, b = ctx.temporal(desc), ctx.temporal(desc)
    try:
        for k, frame in enumerate(frames):
            want, got = a.frame(frame), b.frame_moved(frame, motion)
            assert np.array_equal(bits(got), bits(want)), "frame %d" % k
            assert np.array_equal(bits(b.history()), bits(a.history()))
        assert a.history().max() > 3
    finally:
        a.close()
        b.close()


def test_deformed_mesh_is_reset_and_the_rest_keeps_its_history(pkg, golden):
    import torch
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    mesh = 0
    now = deformed_scene(pkg, scene, mesh, ("wobble", 1))
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=4)
    still = pkg.scene_motion(scene, scene)
    c = pkg.Context(0)
    try:
        c.upload(scene)
        s = c.temporal(pkg.temporal_desc(W, H))
        s.frame_moved(frame, still)
        s.frame_moved(frame, still)
        c.update_meshes(now, [mesh])
        motion = pkg.scene_motion(scene, now, reset_meshes=[mesh])
        assert [i for i in range(len(motion)) if motion["flags"][i] & RESET] == [MESH_NODE] and (motion["flags"] & STATIC).all()
        d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        stream = torch.cuda.Stream(device=0)
        c._check(pkg.hip.rtu_context_sync(c._h))
        s.frame_moved_device(frame, motion, d_out.data_ptr(), stream=stream.cuda_stream)  # the device form, on a caller's stream
        stream.synchronize()
        n = s.history()
        hits = c.frame_features(frame)[0]
        valid = ((hits["flags"] & 1) != 0).reshape(H, W)
        fin = np.isfinite(d_out.cpu().numpy()[..., :3]).all(-1)
        on_mesh = valid & (hits["node"].reshape(H, W) == MESH_NODE)
        rest = valid & ~on_mesh
        assert on_mesh.sum() > 100 and (n[on_mesh & fin] == 1).all(), "a deformed surface kept its history"
        assert (n[rest] == 3).mean() > 0.95, "the rest lost its history"
        # handles stay valid for rtu_temporal_free alone after rtu_destroy_context
        held = pkg.hip.rtu_debug_device_bytes()
        c.close()
        assert pkg.hip.rtu_debug_device_bytes() < held - 212 * W * H + 1, "the session's buffers outlived the context"
        out = np.empty((H, W, 4), F)
        assert pkg.hip.rtu_temporal_frame_moved(s._h, ctypes.byref(frame), motion.ctypes.data, len(motion), 0, out.ctypes.data) == pkg.RTU_ERR_ARG
        s.close()
    finally:
        c.close()
