"""GPU: temporal accumulation for sensors (include/rtu_render.h "Temporal accumulation for sensors"). The device accumulators
(rtu_temporal_accumulate_sensor_device, _sensor_moments_device: k_temporal_sensor<MODEL, MOMENTS>) against their host forms — which
tests/test_sensor_temporal_host.py holds to the rules — bit for bit on the guides of a real scene; a session's sensor frames against
the same frames assembled by hand from the public device entries, byte for byte; the lifetimes of sessions that mix camera and sensor
frames; and what a sensor frame must leave alone."""
import ctypes
import math

import numpy as np
import pytest

from test_gpu_ray_query import bits, materials
from test_gpu_sensor import same_bytes, scene_places
from test_gpu_temporal import dev, hand_frame, orbit_frames
from test_mesh_update_host import clone
from test_sensor_temporal_host import np_temporal_sensor

pytestmark = pytest.mark.gpu

F = np.float32
MODELS = ["equirect", "fisheye", "ortho"]
SIZES = [(64, 32), (33, 17), (48, 48), (40, 30)]  # 33 x 17: ragged, fewer pixels in a row than a workgroup's row of 32 takes twice
SIZE_OF = {"equirect": (64, 32), "fisheye": (48, 48), "ortho": (40, 30)}


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def p10(pkg, golden):
    return golden("p10_s4_160x120").scene(pkg)


@pytest.fixture(scope="module")
def p11(pkg, golden):
    return golden("p11_p2_120x68").scene(pkg)


def moving_sensors(pkg, scene, model, W, H, **recipe):
    """Five sensors in `scene`: an equal pair (STATIC), then a yaw — a panorama's history comes across its seam at every yaw —, a yaw
    with a translation, and a further yaw. The panorama and the fisheye stand inside the scene, the orthographic window at its camera."""
    places, (right, up, fwd), _ = scene_places(pkg, scene)
    dist = float(np.linalg.norm(np.array(places["camera"]) - np.array(places["inside"]))) / 0.8  # from the camera to the centre of the scene's box
    pos = np.array(places["camera" if model == "ortho" else "inside"], np.float64)
    right, up, fwd = (np.array(v, np.float64) for v in (right, up, fwd))
    step = 2 * math.pi * 2.5 / W if model == "equirect" else 0.02
    out = []
    for yaw, shift in ((0.0, 0.0), (0.0, 0.0), (step, 0.0), (2 * step, 0.015), (3.3 * step, 0.015)):
        r2, f2 = right * math.cos(yaw) + fwd * math.sin(yaw), fwd * math.cos(yaw) - right * math.sin(yaw)
        p = pos + shift * dist * (right + 0.5 * up)
        out.append(pkg.sensor_desc(model, W, H, p, r2, up, f2, fov_deg=150.0, extent=(0.8 * dist, 0.8 * dist * H / W), **recipe))
    return out


def centre_guides(pkg, ctx, d):
    """The guides of a sensor frame: ray_features of the pixel-centre rays (the sensor's rays with samples = 0)."""
    c = pkg.RtuSensorDesc.from_buffer_copy(bytes(d))
    c.samples, c.gather_bounces = 0, 0
    return ctx.ray_features(pkg.sensor_rays(c)[0])


# ---- 1. the device forms against the host forms -------------------------------------------------------------------------------------
@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("model", MODELS)
def test_device_forms_equal_the_host_forms(pkg, ctx, p11, model, size, moments):
    import torch
    W, H = size
    planes = 4 if moments else 3
    ctx.upload(p11)
    sensors = moving_sensors(pkg, p11, model, W, H)
    rng = np.random.default_rng(W * 131 + H)
    desc = pkg.temporal_desc(W, H, max_history=3)
    stream = torch.cuda.Stream(device=0)
    hist, d_hist, prev = None, None, None
    lookups = []
    for k, s in enumerate(sensors):
        hits, albedo = centre_guides(pkg, ctx, s)
        rgbz = (rng.random((H, W, 4), dtype=F) * F(2.0)).astype(F)
        rgbz.reshape(-1, 4)[(7 * k + 3) % (W * H), k % 3] = F(np.nan) if k % 2 else F(np.inf)
        want_out, want_hist = pkg.temporal_accumulate_sensor(prev, s, rgbz, hits, albedo, hist, desc, moments=moments)
        lookups.append(np_temporal_sensor(prev, s, rgbz, hits, albedo, hist, desc, moments=moments)[2])
        d_in, d_hits, d_alb = dev(rgbz), dev(hits), dev(albedo)
        d_new = torch.full((planes * H * W * 16 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")  # 64 bytes of guard behind it
        in_place = k == 3
        d_out = d_in if in_place else torch.full((H * W * 16 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
        st = stream if k % 2 else None
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        ctx.temporal_accumulate_sensor_device(desc, prev, s, d_in.data_ptr(), d_hits.data_ptr(), d_alb.data_ptr(),
                                              d_hist.data_ptr() if d_hist is not None else None, d_new.data_ptr(), d_out.data_ptr(), moments=moments,
                                              stream=st.cuda_stream if st else None)
        (st or torch.cuda).synchronize()
        assert pkg.hip.rtu_debug_device_allocations() == a0, "the device form allocated"
        got_out = d_out.cpu().numpy()[:H * W * 16].view(F).reshape(H, W, 4)
        got_hist = d_new.cpu().numpy()
        assert (got_hist[planes * H * W * 16:] == 0x5A).all(), "written past the history"
        if not in_place:
            assert (d_out.cpu().numpy()[H * W * 16:] == 0x5A).all(), "written past the image"
            assert np.array_equal(d_in.cpu().numpy(), rgbz.view(np.uint8).reshape(-1)), "the input was written"
        got_hist = got_hist[:planes * H * W * 16].view(F).reshape(planes, H, W, 4)
        for what, g, w in (("image", got_out, want_out), ("history", got_hist, want_hist)):
            diff = bits(g) != bits(w)
            assert not diff.any(), "%s frame %d %s: %d words differ, first at %s" % (model, k, what, diff.sum(), np.argwhere(diff)[0])
        hist, d_hist, prev = want_hist, d_new, s
    assert [i["lookup"] for i in lookups] == ["none", "static", "reproject", "reproject", "reproject"]
    valid = (hits["flags"] & 1) != 0
    assert valid.mean() > 0.3 and (hist[0][..., 3].reshape(-1)[valid] > 1).mean() > 0.3, "the sensor's moves left no history to speak of"
    if model == "equirect":
        assert sum(int(i["straddle"].sum()) for i in lookups) > 10, "no lookup straddles the seam"


def test_accumulate_device_refusals(pkg, ctx, p10):
    import torch
    W, H = 33, 17
    n = W * H
    buf = torch.zeros(n * (16 + 48 + 16 + 64 + 64 + 16) + 64, dtype=torch.uint8, device="cuda:0")
    base = buf.data_ptr()
    ptrs = [base, base + 16 * n, base + 64 * n, base + 80 * n, base + 144 * n, base + 208 * n]  # rgbz, hits, albedo, hist_prev, hist_out, out
    sensors = moving_sensors(pkg, p10, "fisheye", W, H)
    for fn in (pkg.hip.rtu_temporal_accumulate_sensor_device, pkg.hip.rtu_temporal_accumulate_sensor_moments_device):
        def call(desc, p=ptrs, prev=sensors[2], cur=sensors[3]):
            return fn(ctx._h, ctypes.byref(desc) if desc is not None else None, ctypes.byref(prev) if prev is not None else None,
                      ctypes.byref(cur) if cur is not None else None, *p, None)
        d = pkg.temporal_desc(W, H)
        assert call(d) == pkg.RTU_OK
        for bad in ({"max_history": 0}, {"sigma_plane": 0.0}, {"normal_min": float("nan")}, {"flags": 2}, {"width": 0}, {"width": W + 1}):
            bd = pkg.temporal_desc(W, H)
            for k, v in bad.items():
                setattr(bd, k, v)
            assert call(bd) == pkg.RTU_ERR_ARG, bad
        assert call(None) == pkg.RTU_ERR_ARG and call(d, cur=None) == pkg.RTU_ERR_ARG and call(d, prev=None) == pkg.RTU_ERR_ARG
        for k in range(6):
            p = list(ptrs)
            p[k] = None
            assert call(d, p, prev=None if k == 3 else sensors[2]) == (pkg.RTU_OK if k == 3 else pkg.RTU_ERR_ARG), k  # hist_prev may be NULL
            p[k] = ptrs[k] + 8
            assert call(d, p) == pkg.RTU_ERR_ARG, k
        p = list(ptrs)
        p[4] = ptrs[3] + 16                 # overlapping histories
        assert call(d, p) == pkg.RTU_ERR_ARG
        p = list(ptrs)
        p[5] = ptrs[0]                      # rgbz_out == rgbz is allowed
        assert call(d, p) == pkg.RTU_OK
        bad = moving_sensors(pkg, p10, "fisheye", W, H)[3]
        bad.fov_deg = 400.0
        assert call(d, cur=bad) == pkg.RTU_ERR_ARG and call(d, prev=bad) == pkg.RTU_ERR_ARG
        assert call(d, cur=moving_sensors(pkg, p10, "fisheye", W + 1, H)[3]) == pkg.RTU_ERR_ARG
        assert call(d, prev=moving_sensors(pkg, p10, "ortho", W, H)[2]) == pkg.RTU_OK   # another model: no lookup
        assert fn(None, ctypes.byref(d), ctypes.byref(sensors[2]), ctypes.byref(sensors[3]), *ptrs, None) == pkg.RTU_ERR_ARG
    torch.cuda.synchronize()


# ---- 2. a session's sensor frames against the hand-assembled form ---------------------------------------------------------------------
class Hand:
    """Sensor frames assembled from the public device entries on buffers of the test's own: sensor_rays_device, the shading entry,
    sensor_rays_device of the pixel centres and ray_features_device, temporal_accumulate_sensor_device, and the filter entries."""

    def __init__(self, pkg, ctx, W, H, kind):
        import torch
        self.pkg, self.ctx, self.W, self.H, self.kind = pkg, ctx, W, H, kind
        n = W * H
        self.planes = 4 if kind == "variance" else 3
        z = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
        self.rays, self.keys, self.img, self.hits, self.albedo, self.out, self.var = z(32 * n), z(4 * n), z(16 * n), z(48 * n), z(16 * n), z(16 * n), z(4 * n)
        self.hist = [z(16 * self.planes * n), z(16 * self.planes * n)]
        self.cur, self.prev, self.k = 0, None, 0
        self.desc = pkg.temporal_desc(W, H)
        self.vdesc = pkg.variance_desc(W, H)

    def frame(self, d, take_history=True):
        import torch
        pkg, ctx, n = self.pkg, self.ctx, self.W * self.H
        ctx.sensor_rays_device(d, self.rays.data_ptr(), self.keys.data_ptr(), self.k % d.samples, 1)
        shade = ctx.shade_rays_paths_device if d.gather_bounces else ctx.shade_rays_sampled_device
        for attempt in range(40):  # the capacity repair: a batch that ran out of frame records is shaded again
            shade(self.rays.data_ptr(), self.keys.data_ptr(), n, tuple(d.pos), self.img.data_ptr(), max_bounce=d.max_bounce)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as e:
                assert e.code == pkg.RTU_ERR_CAPACITY
        c = pkg.RtuSensorDesc.from_buffer_copy(bytes(d))
        c.samples, c.gather_bounces = 0, 0
        ctx.sensor_rays_device(c, self.rays.data_ptr(), None, 0, 1)
        ctx.ray_features_device(self.rays.data_ptr(), n, self.hits.data_ptr(), self.albedo.data_ptr())
        prev = self.prev if take_history else None
        new = self.hist[self.cur ^ 1]
        ctx.temporal_accumulate_sensor_device(self.desc, prev, d, self.img.data_ptr(), self.hits.data_ptr(), self.albedo.data_ptr(),
                                              self.hist[self.cur].data_ptr() if prev is not None else None, new.data_ptr(), self.out.data_ptr(),
                                              moments=self.kind == "variance")
        self.cur ^= 1
        self.prev, self.k = d, self.k + 1
        if self.kind == "variance":
            ctx.variance_device(self.vdesc, new.data_ptr(), self.hits.data_ptr(), self.var.data_ptr())
            ctx.denoise_variance_device(self.vdesc, self.out.data_ptr(), self.hits.data_ptr(), self.albedo.data_ptr(), self.var.data_ptr(), self.out.data_ptr())
        elif self.kind == "denoise":
            ctx.denoise_device(pkg.denoise_desc(self.W, self.H), self.out.data_ptr(), self.hits.data_ptr(), self.albedo.data_ptr(), self.out.data_ptr())
        torch.cuda.synchronize()
        return self.out.cpu().numpy().view(F).reshape(self.H, self.W, 4), new.cpu().numpy().view(F).reshape(self.planes, self.H, self.W, 4)


def open_session(pkg, ctx, W, H, kind):
    return ctx.temporal(pkg.temporal_desc(W, H, denoise=kind == "denoise"), variance=pkg.variance_desc(W, H) if kind == "variance" else None)


CASES = [("p10_s4_160x120", 0, kind) for kind in ("plain", "denoise", "variance")] + [("p11_p2_120x68", 4, "plain")]


@pytest.mark.parametrize("tag,gather,kind", CASES, ids=["S-plain", "S-denoise", "S-variance", "P-plain"])
@pytest.mark.parametrize("model", MODELS)
def test_session_equals_the_hand_form(pkg, ctx, golden, model, tag, gather, kind):
    scene = golden(tag).scene(pkg)
    W, H = (33, 17) if (model, kind) == ("fisheye", "denoise") else SIZE_OF[model]
    ctx.upload(scene)
    s = open_session(pkg, ctx, W, H, kind)
    hand = Hand(pkg, ctx, W, H, kind)
    try:
        assert not s.history().any()
        for k in range(5):
            samples = 4 if k < 3 else 2   # S changes mid-session: sample k mod S of the S of that call
            d = moving_sensors(pkg, scene, model, W, H, samples=samples, gather_bounces=gather)[k]
            got = s.sensor_frame(d)
            want, hist = hand.frame(d)
            diff = bits(got) != bits(want)
            assert not diff.any(), "%s frame %d: %d words differ, first at %s" % (model, k, diff.sum(), np.argwhere(diff)[0])
            assert same_bytes(s.history(), np.ascontiguousarray(hist[0][..., 3]))
        n = hist[0][..., 3]
        assert (n > 1).mean() > 0.2 and n.max() > 3, "the sensor's moves left no history to speak of"
        assert (n != np.round(n)).any(), "no pixel was resampled"
    finally:
        s.close()


# ---- 3. lifetimes -------------------------------------------------------------------------------------------------------------------
LW, LH = 64, 32


def camera_frames(pkg, scene, n, **kw):
    return orbit_frames(pkg, scene, LW, LH, n, 20.0, 0.5, **kw)


def test_camera_and_sensor_frames_alternate(pkg, ctx, p10):
    """camera, camera, sensor, sensor, camera, camera on a plain session: each switch takes no history, k goes on counting (sample
    k mod S), and within a kind the history is kept. Against hand forms; a recipe W sensor in between is refused and changes nothing."""
    ctx.upload(p10)
    cams = camera_frames(pkg, p10, 6, samples=4)
    sens = moving_sensors(pkg, p10, "equirect", LW, LH, samples=4)
    desc = pkg.temporal_desc(LW, LH)
    s = ctx.temporal(desc)
    hand = Hand(pkg, ctx, LW, LH, "plain")
    try:
        prev = hist = None
        for k, kind in enumerate(("cam", "cam", "sen", "sen", "cam", "cam")):
            if kind == "cam":
                got = s.frame(cams[k])
                want, hist, _ = hand_frame(pkg, ctx, cams[k], k, prev, hist, desc, False)
                prev, n_want = cams[k], hist[0][..., 3]
                hand.prev = None
            else:
                if k == 3:  # a refused call leaves the session as it was
                    before = s.history()
                    w = moving_sensors(pkg, p10, "equirect", LW, LH, samples=0)[k]
                    with pytest.raises(pkg.RtuError) as e:
                        s.sensor_frame(w)
                    assert e.value.code == pkg.RTU_ERR_ARG and same_bytes(s.history(), before)
                got = s.sensor_frame(sens[k])
                hand.k = k
                want, h = hand.frame(sens[k])
                prev = hist = None
                n_want = h[0][..., 3]
            assert same_bytes(got, want), "frame %d (%s)" % (k, kind)
            assert same_bytes(s.history(), np.ascontiguousarray(n_want))
            if k in (2, 4):
                assert s.history().max() == 1, "the first frame of another kind took a history"
            if k in (1, 3, 5):
                assert s.history().max() > 1, "the second frame of a kind took none"
    finally:
        s.close()


@pytest.mark.parametrize("kind", ["plain", "variance"])
def test_models_scene_updates_resets_and_allocations(pkg, p10, kind):
    c = pkg.Context(0)
    try:
        c.upload(p10)
        eq = moving_sensors(pkg, p10, "equirect", LW, LH, samples=2)
        fe = moving_sensors(pkg, p10, "fisheye", LW, LH, samples=2)
        cams = camera_frames(pkg, p10, 2, samples=2)
        s, hand = open_session(pkg, c, LW, LH, kind), Hand(pkg, c, LW, LH, kind)
        s.frame(cams[0])
        hand.k = 1                                                 # the sensor frame after a camera frame: frame 1, no history
        assert same_bytes(s.sensor_frame(eq[0]), hand.frame(eq[0], take_history=False)[0]) and s.history().max() == 1
        a0 = pkg.hip.rtu_debug_device_allocations()
        assert same_bytes(s.sensor_frame(eq[2]), hand.frame(eq[2])[0]) and s.history().max() > 1
        s.frame(cams[1])
        hand.k = 4
        assert same_bytes(s.sensor_frame(eq[3]), hand.frame(eq[3], take_history=False)[0])
        assert pkg.hip.rtu_debug_device_allocations() == a0, "a frame after the first of its kind allocated"
        # a sensor of another model: no history, k goes on
        got, (want, h) = s.sensor_frame(fe[2]), hand.frame(fe[2], take_history=False)
        assert same_bytes(got, want) and s.history().max() == 1
        assert same_bytes(s.sensor_frame(fe[3]), hand.frame(fe[3])[0]) and s.history().max() > 1
        # reset: the next frame is frame 0 again
        s.reset()
        assert not s.history().any()
        fresh, fhand = open_session(pkg, c, LW, LH, kind), Hand(pkg, c, LW, LH, kind)
        first = fresh.sensor_frame(eq[0])
        assert same_bytes(s.sensor_frame(eq[0]), first) and same_bytes(first, fhand.frame(eq[0])[0])
        s.sensor_frame(eq[2])
        # a new scene: the next frame starts over — no history, sample 0
        painted = clone(pkg, p10)
        for m in range(painted.desc.n_materials):
            materials(painted)[m].diffuse[0] = 0.9
        c.update(painted)
        assert not s.history().any()
        after = s.sensor_frame(eq[3])
        assert s.history().max() == 1
        other = open_session(pkg, c, LW, LH, kind)
        assert same_bytes(other.sensor_frame(eq[3]), after), "after an update the session is not a new one's"
        for x in (s, fresh, other):
            x.close()
    finally:
        c.close()


REFUSING = {"steered": dict(steer=True), "gradient": dict(gradient=True), "sparse": dict(sparse=True), "holes": dict(sparse=True, holes=True)}


@pytest.mark.parametrize("kind", list(REFUSING))
def test_other_sessions_refuse_a_sensor_and_go_on(pkg, ctx, p10, kind):
    ctx.upload(p10)
    o = REFUSING[kind]
    cams = camera_frames(pkg, p10, 3, samples=2)
    d = moving_sensors(pkg, p10, "equirect", LW, LH, samples=2)[0]

    def begin():
        return ctx.temporal(pkg.temporal_desc(LW, LH), variance=pkg.variance_desc(LW, LH),
                            steer=pkg.steer_desc(budget=LW * LH // 2, max_extra=3) if o.get("steer") else None,
                            gradient=pkg.gradient_desc(radius=1, kappa=0.5) if o.get("gradient") else None,
                            sparse=pkg.sparse_desc(block=2) if o.get("sparse") else None,
                            holes=pkg.hole_desc(budget=LW * LH // 8) if o.get("holes") else None)
    a, b = begin(), begin()
    try:
        for k, f in enumerate(cams):
            want = a.frame(f)
            if k > 0:
                before = b.history()
                with pytest.raises(pkg.RtuError) as e:
                    b.sensor_frame(d)
                assert e.value.code == pkg.RTU_ERR_ARG and same_bytes(b.history(), before)
            assert same_bytes(b.frame(f), want), "%s: frame %d after a refused sensor frame" % (kind, k)
            assert same_bytes(a.history(), b.history())
    finally:
        a.close()
        b.close()


def test_session_refusals(pkg, p10):
    import torch
    c = pkg.Context(0)
    try:
        s = c.temporal(pkg.temporal_desc(LW, LH))
        d = moving_sensors(pkg, p10, "equirect", LW, LH, samples=2)[0]
        with pytest.raises(pkg.RtuError) as e:      # before an upload
            s.sensor_frame(d)
        assert e.value.code == pkg.RTU_ERR_NO_SCENE
        c.upload(p10)
        out = np.zeros((LH, LW, 4), F)
        d_out = torch.zeros((LH, LW, 4), dtype=torch.float32, device="cuda:0")
        fn, fd = pkg.hip.rtu_temporal_sensor_frame, pkg.hip.rtu_temporal_sensor_frame_device
        bad = [moving_sensors(pkg, p10, "equirect", LW, LH, samples=0)[0], moving_sensors(pkg, p10, "equirect", LW + 1, LH, samples=2)[0],
               moving_sensors(pkg, p10, "equirect", LW, LH, samples=0, gather_bounces=4)[0]]
        for field, value in (("model", 5), ("max_bounce", 9), ("flags", 8), ("samples", 70000)):
            x = moving_sensors(pkg, p10, "fisheye", LW, LH, samples=2)[0]
            setattr(x, field, value)
            bad.append(x)
        for x in bad:
            assert fn(s._h, ctypes.byref(x), out.ctypes.data) == pkg.RTU_ERR_ARG
        assert fn(s._h, None, out.ctypes.data) == pkg.RTU_ERR_ARG and fn(s._h, ctypes.byref(d), None) == pkg.RTU_ERR_ARG
        assert fn(None, ctypes.byref(d), out.ctypes.data) == pkg.RTU_ERR_ARG
        assert fd(s._h, ctypes.byref(d), None, None) == pkg.RTU_ERR_ARG and fd(s._h, ctypes.byref(d), d_out.data_ptr() + 8, None) == pkg.RTU_ERR_ARG
        assert not s.history().any(), "a refused frame counted"
        want = s.sensor_frame(d)
        # the device form on a caller's stream
        t = c.temporal(pkg.temporal_desc(LW, LH))
        stream = torch.cuda.Stream(device=0)
        c._check(pkg.hip.rtu_context_sync(c._h))
        t.sensor_frame_device(d, d_out.data_ptr(), stream.cuda_stream)
        stream.synchronize()
        assert same_bytes(d_out.cpu().numpy(), want)
        t.close()
        c.close()
        assert fn(s._h, ctypes.byref(d), out.ctypes.data) == pkg.RTU_ERR_ARG  # the context is gone: the handle is good for free alone
        s.close()
    finally:
        c.close()


# ---- 4. it disturbs nothing -------------------------------------------------------------------------------------------------------
def test_an_open_progressive_session_and_a_sensor_render_are_not_disturbed(pkg, ctx, p10):
    ctx.upload(p10)
    f = pkg.frame_setup(p10.desc.camera, 96, 72, samples=4)
    still = moving_sensors(pkg, p10, "equirect", 48, 24, samples=3)[0]
    sens = moving_sensors(pkg, p10, "equirect", LW, LH, samples=4)
    p = ctx.progressive(f)
    s = ctx.temporal(pkg.temporal_desc(LW, LH, denoise=True))
    try:
        p.advance(2)
        snap0, _ = p.snapshot()
        img = ctx.render_sensor(still)
        first = s.sensor_frame(sens[0])
        snap1, _ = p.snapshot()
        assert same_bytes(snap0, snap1) and p.status()[0] == 2
        assert same_bytes(ctx.render_sensor(still), img)
        s.sensor_frame(sens[2])
        p.advance(2)
        assert same_bytes(p.snapshot()[0], ctx.render(f)[0])
        assert same_bytes(ctx.render_sensor(still), img)
        t = ctx.temporal(pkg.temporal_desc(LW, LH, denoise=True))
        assert same_bytes(t.sensor_frame(sens[0]), first), "renders and a progressive session changed a session's frame"
        t.close()
    finally:
        p.close()
        s.close()
