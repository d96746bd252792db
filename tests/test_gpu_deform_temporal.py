"""GPU: temporal accumulation on deforming meshes (include/rtu_render.h). The device accumulators and motion vectors
(k_temporal_deform<MOMENTS>, k_motion_vectors_deform), which read the context's own connectivity and the previous vertices it kept,
against the host forms, which read them from the previous Scene (tests/test_deform_temporal_host.py holds those to the rule), bit for
bit, on the exact surface records of the walk (rtu_frame_surface); the history a deforming teapot keeps over a chain of updates
against the RESET chain; what rtu_keep_previous_vertices allocates and when "previous" is "current"; the refusals."""
import ctypes

import numpy as np
import pytest

from test_gpu_ray_query import bits, frame_of
from test_gpu_temporal import dev
from test_mesh_update_host import clone, deformed_scene

pytestmark = pytest.mark.gpu

F = np.float32
DEFORM = 4
TAGS = ["p5low_200x150", "p10_s4_160x120"]  # the low teapot twice (two nodes of mesh 0) in a closed room; the teapot among spheres


def sample_of(albedo, hits, W, H, seed):
    """A noisy sample of a frame whose guides are (hits, albedo): the albedo under a random light per pixel, z = t."""
    rng = np.random.default_rng(seed)
    rgb = albedo[:, :3] * rng.uniform(0.2, 1.8, (W * H, 3)).astype(F)
    return np.concatenate([rgb, hits["t"][:, None]], axis=1).reshape(H, W, 4).astype(F)


def device_accumulate(pkg, ctx, desc, prev_cam, cur_cam, rgbz, hits, albedo, surf, hist_prev, table, cap, moments, stream=None):
    import torch
    H, W = rgbz.shape[:2]
    planes = 4 if moments else 3
    d_in, d_hits, d_alb, d_surf, d_tab = dev(rgbz), dev(hits), dev(albedo), dev(surf), dev(table)
    d_prev = dev(hist_prev) if hist_prev is not None else None
    d_hist = torch.full((planes * H * W * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d_out = torch.full((H * W * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
    d = pkg.temporal_desc(W, H)
    ctypes.memmove(ctypes.byref(d), ctypes.byref(desc), ctypes.sizeof(d))
    d.width, d.height = W, H
    torch.cuda.synchronize()
    ctx.temporal_accumulate_deform_device(d, prev_cam, cur_cam, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_surf.data_ptr(),
                                          d_prev.data_ptr() if d_prev is not None else None, d_hist.data_ptr(), d_out.data_ptr(), d_tab.data_ptr(),
                                          len(table), cap, moments=moments, stream=stream.cuda_stream if stream else None)
    torch.cuda.synchronize()
    assert np.array_equal(d_surf.cpu().numpy(), np.ascontiguousarray(surf).view(np.uint8).reshape(-1)), "the records were written"
    return d_out.cpu().numpy().view(F).reshape(H, W, 4), d_hist.cpu().numpy().view(F).reshape(planes, H, W, 4)


def same(got, want, what):
    for name, g, w in (("image", got[0], want[0]), ("history", got[1], want[1])):
        diff = bits(g) != bits(w)
        assert not diff.any(), "%s %s: %d words differ, first at %s" % (what, name, diff.sum(), np.argwhere(diff)[0])


def moved_camera(pkg, scene, W, H, dx):
    s = clone(pkg, scene)
    s.desc.camera.pos[0] += dx
    s.desc.camera.pos[2] += 0.5 * dx
    return pkg.frame_setup(s.desc.camera, W, H)


# ---- 1. device against host; the history a deforming mesh keeps ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_device_forms_equal_the_host_forms_over_a_chain_of_updates(pkg, golden, tag):
    import torch
    g = golden(tag)
    base = g.scene(pkg)
    W, H = g.width, g.height
    desc = pkg.temporal_desc(W, H, sigma_plane=0.1, normal_min=0.8)
    ctx = pkg.Context(0)
    stream = torch.cuda.Stream(device=0)
    try:
        ctx.keep_previous_vertices(True)
        scenes = [deformed_scene(pkg, base, 0, ("wobble", k)) for k in range(5)]  # the teapot a step further each frame
        cams = [moved_camera(pkg, base, W, H, 0.15 * k) for k in range(5)]          # and the camera moves too
        ctx.upload(scenes[0])
        hist = {}   # chain -> history
        n_nodes = base.desc.n_nodes
        mesh_px = None
        for k in range(5):
            if k:
                ctx.update_meshes(scenes[k], [0])
            hits, albedo, surf = ctx.frame_surface(cams[k])
            rgbz = sample_of(albedo, hits, W, H, 100 + k)
            tables = {"deform": pkg.scene_motion(scenes[k - 1], scenes[k], deform_meshes=[0]) if k else pkg.scene_motion(scenes[0], scenes[0]),
                      "reset": pkg.scene_motion(scenes[k - 1], scenes[k], reset_meshes=[0]) if k else pkg.scene_motion(scenes[0], scenes[0])}
            prev_scene, prev_cam = (scenes[k - 1], cams[k - 1]) if k else (scenes[0], None)
            for moments in (False, True):
                for chain in ("deform", "reset"):
                    key = (chain, moments)
                    cap = 0 if k % 2 else 6
                    want = pkg.temporal_accumulate_deform(prev_cam, cams[k], rgbz, hits, albedo, surf, prev_scene, tables[chain], hist.get(key), desc,
                                                          cap, moments=moments)
                    got = device_accumulate(pkg, ctx, desc, prev_cam, cams[k], rgbz, hits, albedo, surf, hist.get(key), tables[chain], cap, moments,
                                            stream if k % 2 else None)
                    same(got, want, "%s frame %d %s moments %s" % (tag, k, chain, moments))
                    hist[key] = want[1]
            if k:
                assert (tables["deform"]["flags"] == DEFORM).sum() >= 1
                # the motion vectors, device against host
                d_hits, d_surf, d_tab = dev(hits), dev(surf), dev(tables["deform"])
                d_mv = torch.zeros(W * H * 16, dtype=torch.uint8, device="cuda:0")
                ctx.motion_vectors_deform_device(desc, cams[k - 1], d_hits.data_ptr(), d_surf.data_ptr(), d_tab.data_ptr(), n_nodes, d_mv.data_ptr())
                torch.cuda.synchronize()
                mv = pkg.motion_vectors_deform(cams[k - 1], hits, surf, scenes[k - 1], tables["deform"], W, H)
                assert np.array_equal(bits(d_mv.cpu().numpy().view(F).reshape(H, W, 4)), bits(mv))
                on_mesh = surf["mesh"] == 0
                assert mv.reshape(-1, 4)[on_mesh, 2].mean() > 0.95, "a deforming pixel has a motion vector"
            mesh_px = surf["mesh"] == 0
        n_def = hist[("deform", False)][0][..., 3].reshape(-1)[mesh_px]
        n_res = hist[("reset", False)][0][..., 3].reshape(-1)[mesh_px]
        print("%s: %d teapot pixels; after 4 deformed frames history >= 3 at %.1f %%, mean %.2f; RESET chain: max %g" %
              (tag, mesh_px.sum(), 100 * (n_def >= 3).mean(), n_def.mean(), n_res.max()))
        assert mesh_px.sum() > 500
        assert (n_def >= 3).mean() > 0.9, "the deforming teapot keeps its history"
        assert (n_res == 1).all(), "the RESET chain restarts every pixel of the teapot"
        rest = ~mesh_px.reshape(H, W)
        assert np.array_equal(bits(hist[("deform", False)][0][rest]), bits(hist[("reset", False)][0][rest])), "every other pixel is the motion form's"
    finally:
        ctx.close()


# ---- 2. what the switch keeps and allocates; when previous is current -------------------------------------------------------------------------
def test_previous_vertices_allocation_and_lifetime(pkg, golden):
    g = golden("p5low_200x150")
    base = g.scene(pkg)
    W, H = 96, 72
    frame = frame_of(pkg, base, W, H)
    wob = [deformed_scene(pkg, base, 0, ("wobble", k)) for k in range(3)]
    desc = pkg.temporal_desc(W, H)
    allocs = pkg.hip.rtu_debug_device_allocations
    ctx, fresh = pkg.Context(0), pkg.Context(0)
    try:
        # off (the default): the existing flow allocates what it did — nothing once the buffers exist
        ctx.upload(base)
        for w in wob:  # (the reference tree's buffer grows to the largest of the three trees: that is the existing flow's own growth)
            ctx.update_meshes(w, [0])
        a0 = allocs()
        ctx.update_meshes(wob[1], [0])
        ctx.update_meshes(wob[0], [0])
        assert allocs() == a0, "updates with the switch off allocate"
        # on: the first update of the mesh grows by one v / vn pair at most, later ones by nothing
        ctx.keep_previous_vertices(True)
        ctx.update_meshes(wob[1], [0])
        assert allocs() - a0 <= 2
        a1 = allocs()
        ctx.update_meshes(wob[2], [0])
        ctx.update_meshes(wob[1], [0])
        assert allocs() == a1, "later updates allocate"
        # what the walks see is a fresh upload's: the new generation is where the kernels read
        fresh.upload(wob[1])
        for a, b in zip(ctx.frame_surface(frame), fresh.frame_surface(frame)):
            assert a.tobytes() == b.tobytes()
        # the accumulator reads wob[2] as previous: the host form on that scene
        hits, albedo, surf = ctx.frame_surface(frame)
        rgbz = sample_of(albedo, hits, W, H, 3)
        hist0 = pkg.temporal_accumulate_motion(None, frame, rgbz, hits, albedo, pkg.scene_motion(base, base), None, desc)[1]
        table = pkg.scene_motion(wob[2], wob[1], deform_meshes=[0])
        a1 = allocs()  # (the other context's upload and the host forms' buffers are behind us)
        got = device_accumulate(pkg, ctx, desc, frame, frame, rgbz, hits, albedo, surf, hist0, table, 0, False)
        a2 = allocs()
        assert a2 - a1 <= 2, "the table of the deform kernels: two small buffers, once"
        same(got, pkg.temporal_accumulate_deform(frame, frame, rgbz, hits, albedo, surf, wob[2], table, hist0, desc), "previous = the update before")
        other = pkg.temporal_accumulate_deform(frame, frame, rgbz, hits, albedo, surf, wob[1], table, hist0, desc)
        assert not np.array_equal(bits(got[1]), bits(other[1])), "previous and current vertices cannot be told apart here"
        device_accumulate(pkg, ctx, desc, frame, frame, rgbz, hits, albedo, surf, np.concatenate([hist0, np.zeros((1, H, W, 4), F)]), table, 0, True)
        ctx.update_meshes(wob[2], [0])
        device_accumulate(pkg, ctx, desc, frame, frame, rgbz, hits, albedo, surf, hist0, table, 0, False)
        assert allocs() == a2, "frames and updates after the first allocate"
        # after rtu_upload_scene previous is current
        ctx.upload(wob[1])
        hits, albedo, surf = ctx.frame_surface(frame)
        got = device_accumulate(pkg, ctx, desc, frame, frame, rgbz, hits, albedo, surf, hist0, table, 0, False)
        same(got, pkg.temporal_accumulate_deform(frame, frame, rgbz, hits, albedo, surf, wob[1], table, hist0, desc), "after an upload")
        # an update that does not list the mesh: previous is current again
        ctx.update_meshes(wob[2], [0])
        ctx.update(wob[2])
        hits, albedo, surf = ctx.frame_surface(frame)
        got = device_accumulate(pkg, ctx, desc, frame, frame, rgbz, hits, albedo, surf, hist0, table, 0, False)
        same(got, pkg.temporal_accumulate_deform(frame, frame, rgbz, hits, albedo, surf, wob[1], table, hist0, desc),
             "rtu_update_scene keeps the previous generation of the last rtu_update_meshes")
    finally:
        ctx.close()
        fresh.close()


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------------------
def test_refusals(pkg, golden):
    import torch
    g = golden("p5low_200x150")
    scene = g.scene(pkg)
    W, H = 16, 8
    n = W * H
    frame = frame_of(pkg, scene, W, H)
    nn = scene.desc.n_nodes
    buf = torch.zeros(n * (16 + 48 + 16 + 32 + 64 + 64 + 16) + nn * 96 + 64, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    offs = np.cumsum([0, 16, 48, 16, 32, 64, 64, 16]) * n  # (histories of four planes: the moments form fits too)
    ptrs = [base + int(o) for o in offs]  # rgbz, hits, albedo, surface, hist_prev, hist_out, out, table
    table = pkg.scene_motion(scene, scene, deform_meshes=[0])
    buf[int(offs[7]):int(offs[7]) + nn * 96] = dev(table)
    d = pkg.temporal_desc(W, H)
    ctx = pkg.Context(0)

    def call(p=ptrs, n_nodes=nn, fn=pkg.hip.rtu_temporal_accumulate_deform_device):
        return fn(ctx._h, ctypes.byref(d), ctypes.byref(frame), ctypes.byref(frame), *p, n_nodes, 0, None)
    try:
        assert call() == pkg.RTU_ERR_NO_SCENE
        ctx.upload(scene)
        assert call() == pkg.RTU_ERR_ARG, "the switch is off"
        ctx.keep_previous_vertices(True)
        assert call() == pkg.RTU_OK and call(fn=pkg.hip.rtu_temporal_accumulate_deform_moments_device) == pkg.RTU_OK
        assert call(n_nodes=nn - 1) == pkg.RTU_ERR_ARG and call(n_nodes=nn + 1) == pkg.RTU_ERR_ARG
        for k in (3, 7):
            p = list(ptrs)
            p[k] = None
            assert call(p=p) == pkg.RTU_ERR_ARG
            p[k] = ptrs[k] + 8
            assert call(p=p) == pkg.RTU_ERR_ARG
        mv = lambda surf=ptrs[3], nodes=nn: pkg.hip.rtu_motion_vectors_deform_device(ctx._h, ctypes.byref(d), ctypes.byref(frame), ptrs[1], surf, ptrs[7],
                                                                                    nodes, ptrs[6], None)
        assert mv() == pkg.RTU_OK and mv(surf=None) == pkg.RTU_ERR_ARG and mv(surf=ptrs[3] + 4) == pkg.RTU_ERR_ARG and mv(nodes=1) == pkg.RTU_ERR_ARG
        ctx.keep_previous_vertices(False)
        assert call() == pkg.RTU_ERR_ARG and mv() == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_keep_previous_vertices(None, 1) == pkg.RTU_ERR_ARG
        torch.cuda.synchronize()
    finally:
        ctx.close()


# ---- 4. the session ------------------------------------------------------------------------------------------------------------------------------
def hand_frame(pkg, ctx, frame, k, prev_cam, prev_scene, hist, desc, kind, vdesc, motion, cap, deformed):
    """Frame k by existing entries on the updated context and the host forms: host rays -> host shading -> frame_surface (a deformed
    frame) or frame_features -> the host accumulator of the frame's kind -> the session's host filter."""
    rays, keys = pkg.camera_sample_rays(frame, k % frame.samples)
    rgbt = ctx.shade_rays_sampled(rays, keys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0].reshape(frame.height, frame.width, 4)
    moments = kind == "variance"
    if deformed:
        hits, albedo, surf = ctx.frame_surface(frame)
        out, hist = pkg.temporal_accumulate_deform(prev_cam, frame, rgbt, hits, albedo, surf, prev_scene, motion, hist, desc, cap, moments=moments)
    else:
        hits, albedo = ctx.frame_features(frame)
        form = pkg.temporal_accumulate_moments if moments else pkg.temporal_accumulate_motion
        out, hist = form(prev_cam, frame, rgbt, hits, albedo, motion, hist, desc, cap)
    if kind == "variance":
        out = pkg.denoise_variance(out, hits, albedo, pkg.variance(hist, hits, vdesc), vdesc)
    elif kind == "denoised":
        out = pkg.denoise(out, hits, albedo)
    return out, hist, hits


@pytest.mark.parametrize("kind", ["plain", "denoised", "variance"])
def test_deformed_session_equals_the_hand_form(pkg, golden, kind):
    g = golden("p10_s4_160x120")
    base = g.scene(pkg)
    W, H = g.width, g.height
    teapot = 7  # the node of mesh 0
    # six frames: plain, deformed, deformed with the camera moved, moved (the teapot translated), deformed, plain at rest
    scenes = [base, deformed_scene(pkg, base, 0, ("wobble", 0)), deformed_scene(pkg, base, 0, ("wobble", 1))]
    scenes[2].desc.camera.pos[0] += 0.3
    scenes.append(clone(pkg, scenes[2]))
    scenes[3].node_translate(teapot, (0.2, 0.0, 0.0))
    scenes.append(deformed_scene(pkg, scenes[3], 0, ("wobble", 2)))
    scenes.append(scenes[4])
    how = ["plain", "deformed", "deformed", "moved", "deformed", "plain"]
    frames = [pkg.frame_setup(s.desc.camera, W, H, samples=3) for s in scenes]
    desc = pkg.temporal_desc(W, H, denoise=kind == "denoised")
    vdesc = pkg.variance_desc(W, H, n_passes=2, min_history=2)
    cap = 5 if kind == "denoised" else 0
    ctx = pkg.Context(0)
    try:
        ctx.keep_previous_vertices(True)
        ctx.upload(scenes[0])
        s = ctx.temporal(desc, variance=vdesc if kind == "variance" else None)
        prev = hist = None
        for k, frame in enumerate(frames):
            if how[k] == "deformed":
                ctx.update_meshes(scenes[k], [0])
                motion = pkg.scene_motion(scenes[k - 1], scenes[k], deform_meshes=[0])
                assert (motion["flags"] == DEFORM).sum() == 1
            elif how[k] == "moved":
                ctx.update(scenes[k])
                motion = pkg.scene_motion(scenes[k - 1], scenes[k])
            else:
                motion = pkg.scene_motion(scenes[k], scenes[k])
            want, hist, hits = hand_frame(pkg, ctx, frame, k, prev, scenes[k - 1] if k else scenes[0], hist, desc, kind, vdesc, motion,
                                          0 if how[k] == "plain" else cap, how[k] == "deformed")  # (a plain frame has no cap)
            a0 = pkg.hip.rtu_debug_device_allocations()
            got = s.frame_deformed(frame, motion, cap) if how[k] == "deformed" else s.frame_moved(frame, motion, cap) if how[k] == "moved" else s.frame(frame)
            grown = pkg.hip.rtu_debug_device_allocations() - a0
            # (the first deformed frame grows the records, 32 B per pixel, and the context's deform table; a variance session's plain frame 0
            # its table; nothing later)
            assert grown == 0 or k <= 1, "frame %d (%s) allocated %d times" % (k, how[k], grown)
            assert k != 1 or grown <= 4
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "%s frame %d (%s): %d words differ, first at %s" % (kind, k, how[k], diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3]))
        on_mesh = ((hits["flags"] & 1) != 0) & (hits["node"] == teapot)
        n = s.history().reshape(-1)
        print("%s session: %d teapot pixels, history >= 4 after six mixed frames on %.1f %%" % (kind, on_mesh.sum(), 100 * (n[on_mesh] >= 4).mean()))
        assert on_mesh.sum() > 500 and (n[on_mesh] >= 4).mean() > 0.8
        s.close()
    finally:
        ctx.close()


def test_session_refusals_leave_the_session_as_it_was(pkg, golden):
    g = golden("p10_s4_160x120")
    base = g.scene(pkg)
    W, H = g.width, g.height
    now = deformed_scene(pkg, base, 0, ("wobble", 1))
    frame = pkg.frame_setup(base.desc.camera, W, H, samples=3)
    motion = pkg.scene_motion(base, now, deform_meshes=[0])
    desc = pkg.temporal_desc(W, H)
    ctx = pkg.Context(0)
    try:
        ctx.upload(base)
        sessions = {"steered": ctx.temporal(desc, variance=pkg.variance_desc(), steer=pkg.steer_desc(budget=W * H // 4)),
                    "gradient": ctx.temporal(desc, variance=pkg.variance_desc(), gradient=pkg.gradient_desc()),
                    "sparse": ctx.temporal(desc, variance=pkg.variance_desc(), sparse=pkg.sparse_desc(block=2)),
                    "holes": ctx.temporal(desc, variance=pkg.variance_desc(), sparse=pkg.sparse_desc(block=2), holes=pkg.hole_desc(budget=W * H // 8)),
                    "plain": ctx.temporal(desc)}
        twin = ctx.temporal(desc)  # the plain session's twin, which no refused call touches
        for s in list(sessions.values()) + [twin]:
            s.frame(frame)
        ctx.update_meshes(now, [0])
        for name, s in sessions.items():
            before = s.history()
            with pytest.raises(pkg.RtuError) as e:  # the switch is off: RTU_ERR_ARG for a session that could; the kind is refused first
                s.frame_deformed(frame, motion)
            assert e.value.code == (pkg.RTU_ERR_ARG if name == "plain" else pkg.RTU_ERR_UNSUPPORTED), name
            assert np.array_equal(bits(s.history()), bits(before))
        ctx.keep_previous_vertices(True)
        ctx.update_meshes(now, [0])
        for name, s in sessions.items():
            if name == "plain":
                continue
            before = s.history()
            with pytest.raises(pkg.RtuError) as e:
                s.frame_deformed(frame, motion)
            assert e.value.code == pkg.RTU_ERR_UNSUPPORTED, name
            assert np.array_equal(bits(s.history()), bits(before))
        plain = sessions["plain"]
        with pytest.raises(pkg.RtuError):
            plain.frame_deformed(frame, motion[:-1])
        with pytest.raises(pkg.RtuError):  # the moved frame still refuses the new flag
            plain.frame_moved(frame, motion)
        got = plain.frame_deformed(frame, motion)
        assert plain.history().max() == 2, "the session adopted the update and kept its history"
        # the frame counter too was left as it was: the frame is sample 1 of 3, as in the twin that saw no refusal
        want = twin.frame_deformed(frame, motion)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(plain.history()), bits(twin.history()))
        fresh = ctx.temporal(desc)
        first = fresh.frame_deformed(frame, motion)  # (sample 0, no history)
        fresh.close()
        assert not np.array_equal(bits(got), bits(first)), "frame 0 and frame 1 cannot be told apart"
        # rtu_destroy_context with open sessions: as for moved frames, the handles stay valid for rtu_temporal_free alone
        ctx.close()
        out = np.empty((H, W, 4), F)
        assert pkg.hip.rtu_temporal_frame_deformed(plain._h, ctypes.byref(frame), motion.ctypes.data, len(motion), 0, out.ctypes.data) == pkg.RTU_ERR_ARG
        for s in list(sessions.values()) + [twin]:
            s.close()
    finally:
        ctx.close()
