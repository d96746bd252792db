"""GPU: temporal accumulation (include/rtu_render.h "Temporal accumulation"). The device ray generator of a recipe-S frame
(rtu_camera_sample_rays_device) against its host form, byte for byte; the device accumulator (rtu_temporal_accumulate_device) against
its host form (which tests/test_temporal_host.py holds to the rules), bit for bit in image and history; a session's frames against
the same thing assembled by hand from existing entries; a static camera against a progressive session; the session's contract."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import SIZES
from test_gpu_ray_query import bits, materials
from test_mesh_update_host import clone
from test_temporal_host import CHAINS, FRAMES, chain_cameras, chain_inputs, host_form, orbit_scene, run_chain

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24  # unit roundoff of binary32


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda:0")


# ---- 1. the device ray generator against the host form ------------------------------------------------------------------------------
def test_camera_sample_rays_device_equals_the_host_form(pkg, golden):
    import torch
    g = golden("p10_s4_160x120")
    lens = clone(pkg, g.scene(pkg))
    lens.desc.camera.dof = 0.4
    lens.desc.camera.focaldist = 20.0
    c = pkg.Context(0)  # no scene is ever uploaded: the entry needs none
    stream = torch.cuda.Stream(device=0)
    try:
        a0 = None
        for scene in (g.scene(pkg), lens):
            for W, H in ((g.width, g.height), (67, 35)):
                frame = pkg.frame_setup(scene.desc.camera, W, H, samples=16)
                assert (frame.dof > 0) == (scene is lens)
                for k, sample in enumerate((0, 15)):
                    want_r, want_k = pkg.camera_sample_rays(frame, sample)
                    d_r = torch.full((W * H * 32,), 0x5A, dtype=torch.uint8, device="cuda:0")
                    d_k = torch.full((W * H * 4,), 0x5A, dtype=torch.uint8, device="cuda:0")
                    torch.cuda.synchronize()
                    if a0 is None:
                        a0 = pkg.hip.rtu_debug_device_allocations()
                    s = stream if k else None
                    c.camera_sample_rays_device(frame, sample, d_r.data_ptr(), d_k.data_ptr(), s.cuda_stream if s else None)
                    (s or torch.cuda).synchronize()
                    assert np.array_equal(d_r.cpu().numpy(), want_r.view(np.uint8).reshape(-1)), "rays of sample %d at %dx%d" % (sample, W, H)
                    assert np.array_equal(d_k.cpu().numpy(), want_k.view(np.uint8).reshape(-1)), "keys of sample %d at %dx%d" % (sample, W, H)
                    if scene is lens:
                        assert len(np.unique(want_r["org"], axis=0)) > 0.9 * W * H
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the entry allocated"
        # the refusals of the host form, and the pointers
        frame = pkg.frame_setup(g.scene(pkg).desc.camera, 67, 35, samples=16)
        d_r = torch.zeros(67 * 35 * 32 + 16, dtype=torch.uint8, device="cuda:0")
        d_k = torch.zeros(67 * 35 * 4 + 16, dtype=torch.uint8, device="cuda:0")
        call = lambda f, s, r, k: pkg.hip.rtu_camera_sample_rays_device(c._h, ctypes.byref(f) if f is not None else None, s, r, k, None)
        assert call(frame, 3, d_r.data_ptr(), d_k.data_ptr()) == pkg.RTU_OK
        for s in (-1, 16):
            assert call(frame, s, d_r.data_ptr(), d_k.data_ptr()) == pkg.RTU_ERR_ARG
        assert call(None, 0, d_r.data_ptr(), d_k.data_ptr()) == pkg.RTU_ERR_ARG
        assert call(frame, 0, None, d_k.data_ptr()) == pkg.RTU_ERR_ARG and call(frame, 0, d_r.data_ptr(), None) == pkg.RTU_ERR_ARG
        assert call(frame, 0, d_r.data_ptr() + 8, d_k.data_ptr()) == pkg.RTU_ERR_ARG
        assert call(frame, 0, d_r.data_ptr(), d_k.data_ptr() + 2) == pkg.RTU_ERR_ARG
        assert call(frame, 0, d_r.data_ptr(), d_k.data_ptr() + 4) == pkg.RTU_OK
        assert call(pkg.frame_setup(g.scene(pkg).desc.camera, 67, 35), 0, d_r.data_ptr(), d_k.data_ptr()) == pkg.RTU_ERR_ARG  # recipe W
        big = pkg.frame_setup(g.scene(pkg).desc.camera, 16384, 4097, samples=1)  # more than 2^26 pixels: refused before anything is written
        assert call(big, 0, d_r.data_ptr(), d_k.data_ptr()) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_camera_sample_rays_device(None, ctypes.byref(frame), 0, d_r.data_ptr(), d_k.data_ptr(), None) == pkg.RTU_ERR_ARG
        torch.cuda.synchronize()
    finally:
        c.close()


# ---- 2. the device accumulator against the host form -------------------------------------------------------------------------------
def device_form(pkg, ctx, streams, in_place_at):
    import torch
    state = {"k": 0, "hist": None}

    def form(prev, cur, rgbz, hits, albedo, hist, desc):
        H, W = rgbz.shape[:2]
        k = state["k"] = 0 if hist is None else state["k"] + 1
        d_in, d_hits, d_alb = dev(rgbz), dev(hits), dev(albedo)
        d_prev = state["hist"] if hist is not None else None
        d_hist = torch.full((3 * H * W * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        in_place = k == in_place_at
        d_out = d_in if in_place else torch.full((H * W * 16,), 0x5A, dtype=torch.uint8, device="cuda:0")
        s = streams[k % 2]
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.temporal_accumulate_device(desc, prev, cur, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(), d_prev.data_ptr() if d_prev is not None else None,
                                       d_hist.data_ptr(), d_out.data_ptr(), s.cuda_stream if s else None)
        (s or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        if not in_place:
            assert np.array_equal(d_in.cpu().numpy(), np.ascontiguousarray(rgbz).view(np.uint8).reshape(-1)), "the input was written"
        if d_prev is not None:
            assert np.array_equal(d_prev.cpu().numpy(), np.ascontiguousarray(hist).view(np.uint8).reshape(-1)), "the previous history was written"
        state["hist"] = d_hist
        return d_out.cpu().numpy().view(F).reshape(H, W, 4), d_hist.cpu().numpy().view(F).reshape(3, H, W, 4)
    return form


@pytest.mark.parametrize("size", SIZES + [(200, 150)], ids=lambda s: "%dx%d" % s)
def test_device_form_equals_the_host_form(pkg, ctx, size):
    import torch
    W, H = size
    stream = torch.cuda.Stream(device=0)
    for ci, (name, over) in enumerate(CHAINS):
        cams = chain_cameras(pkg, W, H)[name]
        frames = chain_inputs(pkg, W, H, 4321 + ci)
        desc = pkg.temporal_desc(W, H, **over)
        want = run_chain(pkg, cams, frames, desc, host_form(pkg))
        got = run_chain(pkg, cams, frames, desc, device_form(pkg, ctx, (None, stream), in_place_at=1 + ci))
        for k in range(FRAMES):
            for what, g, w in (("image", got[k][0], want[k][0]), ("history", got[k][1], want[k][1])):
                diff = bits(g) != bits(w)
                assert not diff.any(), "chain %s %s frame %d %s: %d words differ, first at %s" % (name, over, k, what, diff.sum(), np.argwhere(diff)[0])
        if size != (1, 1):
            assert (want[-1][1][0][..., 3] > 1).any(), "nothing was accumulated"


def test_accumulate_device_refusals(pkg, ctx):
    import torch
    W, H = 7, 5
    n = W * H
    buf = torch.zeros(n * (16 + 48 + 16 + 48 + 48 + 16) + 64, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    ptrs = [base, base + 16 * n, base + 64 * n, base + 80 * n, base + 128 * n, base + 176 * n]  # rgbz, hits, albedo, hist_prev, hist_out, out
    cams = chain_cameras(pkg, W, H)["X"]

    def call(desc, p=ptrs, prev=cams[2], cur=cams[3]):
        return pkg.hip.rtu_temporal_accumulate_device(ctx._h, ctypes.byref(desc) if desc is not None else None, ctypes.byref(prev) if prev is not None else None,
                                                      ctypes.byref(cur) if cur is not None else None, *p, None)
    assert call(pkg.temporal_desc(W, H)) == pkg.RTU_OK
    for bad in ({"max_history": 0}, {"max_history": 65536}, {"sigma_plane": 0.0}, {"sigma_plane": float("nan")}, {"normal_min": 1.5},
                {"normal_min": float("nan")}, {"flags": 2}, {"width": 0}, {"height": -1}, {"width": 8}):
        d = pkg.temporal_desc(W, H)
        for k, v in bad.items():
            setattr(d, k, v)
        assert call(d) == pkg.RTU_ERR_ARG, bad
    d = pkg.temporal_desc(W, H)
    d.reserved[0] = 1
    assert call(d) == pkg.RTU_ERR_ARG
    d = pkg.temporal_desc(W, H)
    assert call(None) == pkg.RTU_ERR_ARG and call(d, cur=None) == pkg.RTU_ERR_ARG and call(d, prev=None) == pkg.RTU_ERR_ARG
    for k in range(6):
        p = list(ptrs)
        p[k] = None
        assert call(d, p, prev=None if k == 3 else cams[2]) == (pkg.RTU_OK if k == 3 else pkg.RTU_ERR_ARG), k  # hist_prev may be NULL
        p[k] = ptrs[k] + 8
        assert call(d, p) == pkg.RTU_ERR_ARG, k
    p = list(ptrs)
    p[4] = ptrs[3]                      # aliased histories
    assert call(d, p) == pkg.RTU_ERR_ARG
    p[4] = ptrs[3] + 16                 # overlapping
    assert call(d, p) == pkg.RTU_ERR_ARG
    p = list(ptrs)
    p[5] = ptrs[0]                      # rgbz_out == rgbz is allowed
    assert call(d, p) == pkg.RTU_OK
    assert pkg.hip.rtu_temporal_accumulate_device(None, ctypes.byref(d), ctypes.byref(cams[2]), ctypes.byref(cams[3]), *ptrs, None) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()


# ---- 3. a session's frames against the hand-assembled form --------------------------------------------------------------------------
def hand_frame(pkg, ctx, frame, k, prev, hist, desc, denoise):
    """Frame k by existing entries: host rays -> host shading -> frame_features -> host accumulator (-> host filter)."""
    rays, keys = pkg.camera_sample_rays(frame, k % frame.samples)
    shade = ctx.shade_rays_paths if frame.gather_bounces else ctx.shade_rays_sampled
    rgbt = shade(rays, keys, tuple(frame.cam_pos), max_bounce=frame.max_bounce)[0].reshape(frame.height, frame.width, 4)
    hits, albedo = ctx.frame_features(frame)
    out, hist = pkg.temporal_accumulate(prev, frame, rgbt, hits, albedo, hist, desc)
    return (pkg.denoise(out, hits, albedo) if denoise else out), hist, hits


def orbit_frames(pkg, scene, W, H, n, distance, step, **kw):
    return [pkg.frame_setup(orbit_scene(pkg, scene, k, distance, step).desc.camera, W, H, **kw) for k in range(n)]


@pytest.mark.parametrize("tag,kw,distance", [("p10_s4_160x120", {"samples": 3}, 20.0), ("p11_p2_120x68", {"samples": 3, "gather_bounces": 4}, 60.0)],
                         ids=["S", "P"])
@pytest.mark.parametrize("denoise", [False, True], ids=["plain", "denoised"])
def test_session_equals_the_hand_form(pkg, ctx, golden, tag, kw, distance, denoise):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    frames = orbit_frames(pkg, scene, W, H, 4, distance, 0.5, **kw)  # samples 0, 1, 2, 0 of S = 3
    desc = pkg.temporal_desc(W, H, denoise=denoise)
    s = ctx.temporal(desc)
    try:
        assert not s.history().any()
        prev = hist = None
        for k, frame in enumerate(frames):
            got = s.frame(frame)
            want, hist, hits = hand_frame(pkg, ctx, frame, k, prev, hist, desc, denoise)
            prev = frame
            diff = bits(got) != bits(want)
            assert not diff.any(), "frame %d: %d words differ, first at %s" % (k, diff.sum(), np.argwhere(diff)[0])
            assert np.array_equal(bits(s.history()), bits(hist[0][..., 3]))
        valid = (hits["flags"] & 1) != 0
        n = hist[0][..., 3].reshape(-1)
        assert (n[valid] > 1).mean() > 0.5 and n.max() > 3, "the camera's moves left no history to speak of"
        assert (n[valid] != np.round(n[valid])).any(), "no pixel was resampled"
    finally:
        s.close()


# ---- 4. a static camera against a progressive session -----------------------------------------------------------------------------
def test_static_camera_against_progressive(pkg, ctx, golden):
    g = golden("p11_p2_120x68")
    scene = g.scene(pkg)
    W, H, K = g.width, g.height, 8
    ctx.upload(scene)
    frame = pkg.frame_setup(scene.desc.camera, W, H, samples=16, gather_bounces=4)
    hits, albedo = ctx.frame_features(frame)
    valid = ((hits["flags"] & 1) != 0).reshape(H, W)
    assert valid.all(), "a closed room: every pixel hits"
    samples = ctx.sample_images(frame, 0, K)[..., :3]
    fin = np.isfinite(samples).all(axis=(0, 3))
    s = ctx.temporal(pkg.temporal_desc(W, H))
    try:
        for k in range(K):
            out = s.frame(frame)
            n = s.history()
            assert np.array_equal(n[fin], np.full(int(fin.sum()), k + 1, F)), "frame %d: history is not exactly %d" % (k, k + 1)
            counted = np.isfinite(samples[:k + 1]).all(axis=3).sum(axis=0)  # a sample that is not finite is not counted
            assert np.array_equal(n, counted.astype(F))
    finally:
        s.close()
    p = ctx.progressive(frame)
    try:
        p.advance(K)
        snap = p.snapshot()[0]
    finally:
        p.close()
    # The bound. With C = max_k |c_k| of a pixel's channel, M = C / d and u = 2^-24: every e_cur = c_k / d is off by u M; blend step
    # k computes e + (e_cur - e) * fl(1 / k): the difference (at most 2 M) rounds once, fl(1 / k) is off by u relatively and the
    # product rounds once — 6 u M / k in all — and the sum (at most M) rounds once, u M; an earlier error enters the next step times
    # (1 - 1 / k) <= 1. In exact arithmetic the recurrence is the mean of the e_cur, so e_K is off by at most
    # u M (1 + sum_k (6 / k + 1)); e * d rounds once more. The snapshot adds K samples in order — K - 1 roundings of partial sums of
    # at most K C — and divides once: u C (K - 1 + 1) in the mean. Second-order terms: a factor 1 + 2^-20.
    Hk = sum(1.0 / k for k in range(1, K + 1))
    C = np.abs(samples.astype(np.float64)).max(axis=0)
    bound = U * C * ((1 + 6 * Hk + K) + 1 + K) * (1 + 2.0 ** -20)
    err = np.abs(out[..., :3].astype(np.float64) - snap[..., :3].astype(np.float64))
    assert fin.mean() > 0.99
    worst = float((err[fin] / np.maximum(bound[fin], 1e-300)).max())
    print("static camera, %d frames: largest error / bound %.3f" % (K, worst))
    assert (err[fin] <= bound[fin]).all(), "largest error / bound %.3f" % worst


# ---- 5. the contract ---------------------------------------------------------------------------------------------------------------
def test_session_contract(pkg, golden):
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    frames = orbit_frames(pkg, scene, W, H, 3, 20.0, 0.5, samples=4)
    plain = pkg.frame_setup(scene.desc.camera, W, H, samples=2)
    desc = pkg.temporal_desc(W, H)
    c = pkg.Context(0)
    try:
        a = c.temporal(desc)
        with pytest.raises(pkg.RtuError) as e:      # before an upload
            a.frame(frames[0])
        assert e.value.code == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        render0 = c.render(plain)[0]
        valid = ((c.frame_features(frames[1])[0]["flags"] & 1) != 0).reshape(H, W)
        b = c.temporal(desc)                        # two sessions on one context
        a0 = a.frame(frames[0])
        a1 = a.frame(frames[1])
        b0 = b.frame(frames[0])
        between = c.render(plain)[0]                # a render between two frames of b ...
        n1 = pkg.hip.rtu_debug_device_allocations()
        b1 = b.frame(frames[1])
        assert pkg.hip.rtu_debug_device_allocations() == n1, "a frame after the first allocated"
        assert np.array_equal(bits(between), bits(render0)), "the session changed a render"
        assert np.array_equal(bits(b0), bits(a0)) and np.array_equal(bits(b1), bits(a1)), "the render changed the session's next frame"
        assert (b.history()[valid] > 1).any()
        # reset: the next frame is frame 0 again
        b.reset()
        assert not b.history().any()
        r0 = b.frame(frames[0])
        assert np.array_equal(bits(r0), bits(a0)) and set(np.unique(b.history()[valid])) <= {0.0, 1.0} and (b.history()[valid] == 1).mean() > 0.99
        # a new scene: no history, and sample 0 again — not stale
        painted = clone(pkg, scene)
        for m in range(painted.desc.n_materials):
            materials(painted)[m].diffuse[0] = 0.9
        c.update(painted)
        assert not a.history().any()
        a2 = a.frame(frames[1])
        assert set(np.unique(a.history()[valid])) <= {0.0, 1.0} and (a.history()[valid] == 1).mean() > 0.99
        fresh = c.temporal(desc)
        assert np.array_equal(bits(fresh.frame(frames[1])), bits(a2)), "after an update the session is not a new one's"
        fresh.close()
        # the refusals
        for bad in (pkg.frame_setup(scene.desc.camera, W + 1, H, samples=4), pkg.frame_setup(scene.desc.camera, W, H),
                    pkg.frame_setup(scene.desc.camera, W, H, shard_rank=0, shard_count=2, samples=4)):
            with pytest.raises(pkg.RtuError) as e:
                a.frame(bad)
            assert e.value.code == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_frame(a._h, None, a0.ctypes.data) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_frame(a._h, ctypes.byref(frames[0]), None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_frame_device(a._h, ctypes.byref(frames[0]), None, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_frame(None, ctypes.byref(frames[0]), a0.ctypes.data) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_history_device(a._h, None, None) == pkg.RTU_ERR_ARG
        for over in ({"max_history": 0}, {"sigma_plane": -1.0}, {"flags": 4}, {"width": 0}):
            bd = pkg.temporal_desc(W, H)
            for k, v in over.items():
                setattr(bd, k, v)
            with pytest.raises(pkg.RtuError) as e:
                c.temporal(bd)
            assert e.value.code == pkg.RTU_ERR_ARG
        err = ctypes.c_int(0)
        assert not pkg.hip.rtu_temporal_begin(None, ctypes.byref(desc), ctypes.byref(err)) and err.value == pkg.RTU_ERR_ARG
        # free after rtu_destroy_context: the handles stay valid for that alone
        held = pkg.hip.rtu_debug_device_bytes()
        c.close()
        assert pkg.hip.rtu_debug_device_bytes() < held - 2 * 212 * W * H + 1, "the sessions' buffers outlived the context"
        assert pkg.hip.rtu_temporal_frame(a._h, ctypes.byref(frames[0]), a0.ctypes.data) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_temporal_reset(a._h) == pkg.RTU_ERR_ARG
        a.close()
        b.close()
    finally:
        c.close()


def test_frame_device_on_a_callers_stream(pkg, ctx, golden):
    import torch
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    W, H = g.width, g.height
    ctx.upload(scene)
    frames = orbit_frames(pkg, scene, W, H, 2, 20.0, 0.5, samples=4)
    desc = pkg.temporal_desc(W, H, denoise=True)
    a, b = ctx.temporal(desc), ctx.temporal(desc)
    stream = torch.cuda.Stream(device=0)
    try:
        d_out = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        d_n = torch.zeros((H, W), dtype=torch.float32, device="cuda:0")
        torch.cuda.synchronize()
        for frame in frames:
            want = a.frame(frame)
            ctx._check(pkg.hip.rtu_context_sync(ctx._h))
            b.frame_device(frame, d_out.data_ptr(), stream.cuda_stream)
            b.history_device(d_n.data_ptr(), stream.cuda_stream)
            stream.synchronize()
            assert np.array_equal(bits(d_out.cpu().numpy()), bits(want))
            assert np.array_equal(bits(d_n.cpu().numpy()), bits(a.history()))
    finally:
        a.close()
        b.close()
