"""Adaptive sensors on the GPU (rtu_render_sensor_adaptive / _device, rtu_debug_sensor_adaptive_trace; include/rtu_render.h, "Adaptive
sensors").

Sample i of a pixel is sample i of the fixed sensor and the sums are formed in sample order, so the image and the counts are compared
bit for bit with the numpy replay of the rule (tests/test_gpu_adaptive.py) on what the existing, oracle-anchored host entries answer to
sensor_rays(desc, k): shade_rays_sampled (recipe S) or shade_rays_paths (recipe P). A sample outside the fisheye circle (t == 0) adds
zeros and is no hit: the replay sees it as a black miss. On p4 the counts and the image are also tied to the oracle's replay of
tests/test_sensor_adaptive_host.py."""
import ctypes

import numpy as np
import pytest

from test_gpu_adaptive import mean_of, mixed_target, replay, same_bits
from test_gpu_parity import check_against
from test_gpu_sensor import glassroom, same_bytes, scene_places
from test_light_lists import RtuLight
from test_gpu_ray_query import lights
from test_mesh_update_host import clone, deformed_scene
from test_sensor_adaptive_host import ORACLE_CASES, adaptive_violations, oracle_case
from test_sensor_host import BIG, camera_basis, make, refusals

pytestmark = pytest.mark.gpu

f32 = np.float32
GATHER = {"p10_s4_160x120": 0, "p11gs_s2_160x90": 0, "p4_240x135": 0, "p11_p2_120x68": 4, "p13_p2_96x72": 4}  # tag -> gather_bounces
SENSORS = {"equirect": ("equirect", 37, 19), "fisheye": ("fisheye", 64, 64), "ortho": ("ortho", 24, 12)}
RULES = [(17, 3, 1), (12, 4, 2)]  # samples, min_samples, increment


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def sensor(pkg, scene, model, W, H, samples, gather=0, where="camera"):
    """The sensor at the scene's camera (or inside its box), looking as the camera does: a fisheye of 360 degrees, an orthographic window
    of half the box's diagonal."""
    places, (right, up, fwd), diag = scene_places(pkg, scene)
    return pkg.sensor_desc(model, W, H, places[where], right, up, fwd, samples=samples, gather_bounces=gather, fov_deg=360.0,
                           extent=(0.5 * diag, 0.25 * diag))


def sample_images(pkg, ctx, d):
    """Per sample what the sensor accumulator adds, [S, H, W, 4], from the host entries: a miss and a sample outside the fisheye circle
    have t = RTU_BIGFLOAT (the latter is black). Also the number of samples outside the circle."""
    imgs = np.empty((d.samples, d.height, d.width, 4), f32)
    eye = tuple(d.pos)
    outside = 0
    for k in range(d.samples):
        rays, keys = pkg.sensor_rays(d, k)
        shade = ctx.shade_rays_paths if d.gather_bounces else ctx.shade_rays_sampled
        out = shade(rays, keys, eye, max_bounce=d.max_bounce)[0].copy()
        zero = out[:, 3] == 0
        assert np.array_equal(zero, (rays["dir"] == 0).all(axis=1)) and not out[zero, :3].any()
        outside += int(zero.sum())
        out[zero, 3] = BIG
        imgs[k] = out.reshape(d.height, d.width, 4)
    return imgs, outside


def check_replay(ctx, d, ad, imgs, what=""):
    got, counts = ctx.render_sensor_adaptive(d, ad)
    ctx.frame_status()
    want, want_counts = replay(imgs, ad.min_samples, ad.increment, ad.target_variance)
    assert np.array_equal(counts, want_counts), "%s: %d pixels stop elsewhere than the replay" % (what, int((counts != want_counts).sum()))
    assert same_bits(got, want), "%s: %d pixels differ from the replay" % (what, int((got.view(np.uint32) != want.view(np.uint32)).any(-1).sum()))
    return got, counts


def schedule(counts, samples, max_batch):
    """The batches of the header's loop for a count map: [(live pixels, samples of the batch)]."""
    out, done = [], 0
    most = max_batch if max_batch else 16
    live = counts.size
    while live:
        nb = min(most, (1 << 25) // live, samples - done)
        out.append((live, nb))
        done += nb
        live = int((counts.astype(np.int64) > done).sum())
    return out


# ---- 1. the replay, bit for bit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(GATHER))
@pytest.mark.parametrize("model", list(SENSORS))
@pytest.mark.parametrize("rule", RULES)
def test_replay(pkg, ctx, golden, tag, model, rule):
    S, mn, inc = rule
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    # (p4 is deterministic, its samples differ by their pixel offsets alone: from inside the box the image has the edges that give its
    # count map a middle; from the camera nine tenths of an equirectangular image are background)
    d = sensor(pkg, scene, *SENSORS[model], samples=S, gather=GATHER[tag], where="inside" if tag == "p4_240x135" else "camera")
    imgs, outside = sample_images(pkg, ctx, d)
    if model == "fisheye":
        assert outside > 0
    ad = pkg.adaptive_defaults(min_samples=mn, increment=inc, target_variance=mixed_target(imgs, mn))
    _, counts = check_replay(ctx, d, ad, imgs, "%s %s %s" % (tag, model, rule))
    values, n = np.unique(counts, return_counts=True)
    print("%s %s %d / %d / %d: counts %s, %d samples outside the circle" % (tag, model, S, mn, inc, dict(zip(values.tolist(), n.tolist())), outside))
    assert values[0] == mn and values[-1] == S and ((values > mn) & (values < S)).any()


# ---- 2. batching changes nothing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p11gs_s2_160x90", "p11_p2_120x68"])
def test_batching_changes_nothing(pkg, ctx, golden, tag):
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    d = sensor(pkg, scene, "equirect", 37, 19, samples=17, gather=GATHER[tag])
    imgs, _ = sample_images(pkg, ctx, d)
    target = mixed_target(imgs, 3)
    ref, ref_counts = check_replay(ctx, d, pkg.adaptive_defaults(min_samples=3, increment=1, target_variance=target), imgs)
    assert len(np.unique(ref_counts)) >= 3
    for B in (1, 3, 16):
        got, counts = ctx.render_sensor_adaptive(d, pkg.adaptive_defaults(min_samples=3, increment=1, target_variance=target, max_batch=B))
        assert np.array_equal(counts, ref_counts) and same_bytes(got, ref), "max_batch %d" % B
        assert ctx.sensor_adaptive_trace() == schedule(ref_counts, 17, B)


# ---- 3. the saving is real ------------------------------------------------------------------------------------------------------------
def test_stopped_pixels_are_not_traced(pkg, ctx, golden):
    scene = golden("p10_s4_160x120").scene(pkg)
    ctx.upload(scene)
    S, mn, inc, B = 17, 3, 1, 4
    target = None
    lives = []
    for W, H in ((37, 19), (1, 1), (63, 1), (64, 1), (65, 1)):
        d = sensor(pkg, scene, "equirect", W, H, samples=S)
        imgs, _ = sample_images(pkg, ctx, d)
        if target is None:
            target = mixed_target(imgs, mn)  # (of the 703 pixels; the same target for the smaller sensors of the same place)
        ad = pkg.adaptive_defaults(min_samples=mn, increment=inc, target_variance=target, max_batch=B)
        _, counts = check_replay(ctx, d, ad, imgs, "%dx%d" % (W, H))
        trace = ctx.sensor_adaptive_trace()
        print("%dx%d: batches (live pixels, samples) %s" % (W, H, trace))
        assert trace == schedule(counts, S, B)
        # each pixel is traced to the end of the batch in which it stopped
        n = counts.astype(np.int64)
        assert sum(l * b for l, b in trace) == int(np.minimum(S, B * ((n + B - 1) // B)).sum())
        if W * H == 703:
            assert sum(l * b for l, b in trace) < S * W * H
        lives += [l for l, _ in trace]
    assert any(l % 64 for l in lives) and any(l < 64 for l in lives) and any(l > 256 for l in lives)


# ---- 4. limits ------------------------------------------------------------------------------------------------------------------------
def test_limits(pkg, ctx, golden):
    scene = golden("p11gs_s2_160x90").scene(pkg)
    ctx.upload(scene)
    S = 12
    d = sensor(pkg, scene, "fisheye", 32, 32, samples=S)
    imgs, outside = sample_images(pkg, ctx, d)
    assert outside > 0
    fixed = ctx.render_sensor(d)
    img, counts = ctx.render_sensor_adaptive(d, pkg.adaptive_defaults(min_samples=S, increment=1, target_variance=0.0))
    assert (counts == S).all() and same_bytes(img, fixed)
    assert ctx.sensor_adaptive_trace() == [(32 * 32, S)]
    img, counts = ctx.render_sensor_adaptive(d, pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=float("inf")))
    assert (counts == 4).all() and same_bits(img, mean_of(imgs, 4))
    # a target of 0: only pixels whose variance is exactly 0 stop early (the pixels outside the circle among them)
    ad0 = pkg.adaptive_defaults(min_samples=4, increment=2, target_variance=0.0)
    _, counts = check_replay(ctx, d, ad0, imgs, "target 0")
    assert (counts == 4).any() and (counts == S).any()
    # min_samples 1: the checkpoint at n == 1 has var = +inf and never passes a finite target
    _, counts = check_replay(ctx, d, pkg.adaptive_defaults(min_samples=1, increment=1, target_variance=mixed_target(imgs, 2)), imgs, "min_samples 1")
    assert counts.min() == 2
    img, counts = ctx.render_sensor_adaptive(d, pkg.adaptive_defaults(min_samples=1, increment=1, target_variance=float("inf")))
    assert (counts == 1).all() and same_bits(img, mean_of(imgs, 1))


@pytest.mark.parametrize("samples", [1, 255])
def test_the_ends_of_the_sample_range(pkg, ctx, golden, samples):
    scene = golden("p10_s4_160x120").scene(pkg)
    ctx.upload(scene)
    d = sensor(pkg, scene, "equirect", 8, 4, samples=samples)
    imgs, _ = sample_images(pkg, ctx, d)
    mn = min(samples, 8)
    target = 0.0 if samples == 1 else mixed_target(imgs, mn)
    _, counts = check_replay(ctx, d, pkg.adaptive_defaults(min_samples=mn, increment=1, target_variance=target), imgs)
    assert counts.max() == samples or samples == 255
    assert same_bytes(ctx.render_sensor_adaptive(d, pkg.adaptive_defaults(min_samples=samples))[0], ctx.render_sensor(d))


# ---- 5. the oracle ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_against_the_oracle(pkg, orc, ctx, golden, name):
    c = oracle_case(pkg, orc, golden, name)
    ctx.upload(c["scene"])
    got, counts = ctx.render_sensor_adaptive(c["desc"], c["adaptive"])
    clear = c["margin"] >= 1e-3
    differ = counts != c["counts"]
    print("p4 %s: %d pixels, %d borderline, %d differ in count" % (name, differ.size, int((~clear).sum()), int(differ.sum())))
    assert not (differ & clear).any(), "%d pixels stop elsewhere than the oracle, clear of the target" % int((differ & clear).sum())
    # the image at the device's counts against the oracle's mean of each pixel's first n samples
    cpu = np.empty_like(got)
    for n in np.unique(counts):
        at = counts == n
        cpu[at] = mean_of(c["imgs"], int(n))[at]
    check_against(got, cpu, orc)


# ---- 6. the contract --------------------------------------------------------------------------------------------------------------------
def test_capacity_overflow_inside_a_batch(pkg, tmp_path):
    scene = glassroom(pkg, tmp_path)
    W, H = 128, 96
    d = pkg.sensor_desc("ortho", W, H, (0.0, -14.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), samples=4, extent=(12.0, 9.0))
    other = pkg.Context(0)
    try:
        other.upload(scene)
        imgs, _ = sample_images(pkg, other, d)
    finally:
        other.close()
    # (in this window the room's samples agree exactly, so there is no mixed target: the checkpoint lies inside the second batch, and
    # whatever stops there stops mid-batch)
    ad = pkg.adaptive_defaults(min_samples=3, increment=1, target_variance=0.0, max_batch=2)
    c = pkg.Context(0)  # a fresh context: nothing learned, nothing grown
    try:
        c.upload(scene)
        _, counts = check_replay(c, d, ad, imgs, "first")
        frames, _ = c.frame_counts()
        assert max(frames[1:]) > 2 * W * H, frames  # more child frames in some level than the first batch has rays: it did overflow
        assert c.sensor_adaptive_trace() == schedule(counts, 4, 2) and (counts == 3).any()
        check_replay(c, d, ad, imgs, "second")
    finally:
        c.close()


def p10_sensor(pkg, scene, samples=6, W=48, H=24):
    pos, right, up, fwd = camera_basis(scene)
    return pkg.sensor_desc("equirect", W, H, pos, right, up, fwd, samples=samples)


def test_it_disturbs_nothing_and_allocates_once(pkg, golden):
    scene = golden("p10_s4_160x120").scene(pkg)
    c = pkg.Context(0)
    try:
        c.upload(scene)
        frame = pkg.frame_setup(scene.desc.camera, 96, 72, samples=4)
        d = p10_sensor(pkg, scene)
        ad = pkg.adaptive_defaults(min_samples=2, increment=1, target_variance=1e-3, max_batch=2)
        before = c.render(frame)[0]
        fixed = c.render_sensor(d)
        p = c.progressive(frame)
        try:
            p.advance(2)
            snap = p.snapshot()[0]
            img, counts = c.render_sensor_adaptive(d, ad)
            assert len(np.unique(counts)) >= 2
            a0 = pkg.hip.rtu_debug_device_allocations()
            for _ in range(5):
                again, again_counts = c.render_sensor_adaptive(d, ad)
                assert same_bytes(again, img) and np.array_equal(again_counts, counts)
            assert pkg.hip.rtu_debug_device_allocations() == a0  # repeated renders of one shape allocate nothing
            assert same_bytes(p.snapshot()[0], snap) and p.status()[0] == 2
            p.advance(2)
            assert same_bytes(p.snapshot()[0], before)
        finally:
            p.close()
        assert same_bytes(c.render(frame)[0], before) and same_bytes(c.render_sensor(d), fixed)
    finally:
        c.close()


def test_it_follows_scene_updates(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    pos, right, up, fwd = camera_basis(scene)
    d = pkg.sensor_desc("fisheye", 48, 48, pos, right, up, fwd, samples=6, fov_deg=60.0)
    ad = pkg.adaptive_defaults(min_samples=2, increment=2, target_variance=1e-4)

    def fresh(s):
        f = pkg.Context(0)
        try:
            f.upload(s)
            return f.render_sensor_adaptive(d, ad)
        finally:
            f.close()

    def same(a, b):
        return same_bytes(a[0], b[0]) and np.array_equal(a[1], b[1])
    c = pkg.Context(0)
    try:
        c.upload(scene)
        out0 = c.render_sensor_adaptive(d, ad)
        assert len(np.unique(out0[1])) >= 2
        relit = clone(pkg, scene)
        l = RtuLight.from_buffer_copy(bytes(lights(relit)[1]))
        l.vec[0], l.vec[1], l.vec[2] = l.vec[0] + 0.5, l.vec[1] - 0.25, l.vec[2]
        relit.set_light(1, l)
        c.update(relit)
        out1 = c.render_sensor_adaptive(d, ad)
        assert not same_bytes(out1[0], out0[0]) and same(out1, fresh(relit))
        twisted = deformed_scene(pkg, relit, 0, ("twist", 120))
        c.update_meshes(twisted, [0])
        out2 = c.render_sensor_adaptive(d, ad)
        assert not same_bytes(out2[0], out1[0]) and same(out2, fresh(twisted))
    finally:
        c.close()


def test_the_device_form_on_a_callers_stream_and_two_contexts(pkg, ctx, golden):
    import torch
    scene = golden("p11gs_s2_160x90").scene(pkg)
    ctx.upload(scene)
    pos, right, up, fwd = camera_basis(scene)
    other = pkg.Context(0)
    try:
        other.upload(scene)
        stream = torch.cuda.Stream(device=0)
        for gather in (0, 4):
            d = pkg.sensor_desc("equirect", 40, 20, pos, right, up, fwd, samples=6, gather_bounces=gather)
            target = mixed_target(sample_images(pkg, ctx, d)[0], 2)
            ad = pkg.adaptive_defaults(min_samples=2, increment=1, target_variance=target, max_batch=3)
            host, counts = ctx.render_sensor_adaptive(d, ad)
            assert len(np.unique(counts)) >= 2
            d_out = torch.full((40 * 20 * 4 + 16,), 7.0, dtype=torch.float32, device="cuda:0")
            d_counts = torch.full((40 * 20 + 16,), 77, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            ctx.render_sensor_adaptive_device(d, d_out.data_ptr(), d_counts.data_ptr(), ad, stream.cuda_stream)  # returns when the image is complete
            ctx.frame_status()
            dev, dc = d_out.cpu().numpy(), d_counts.cpu().numpy()
            assert same_bytes(dev[:-16].reshape(20, 40, 4), host) and (dev[-16:] == 7.0).all()
            assert np.array_equal(dc[:-16].reshape(20, 40), counts) and (dc[-16:] == 77).all()
            d_out.fill_(7.0)
            torch.cuda.synchronize()
            ctx.render_sensor_adaptive_device(d, d_out.data_ptr(), None, ad, stream.cuda_stream)  # without counts
            assert same_bytes(d_out.cpu().numpy()[:-16].reshape(20, 40, 4), host)
            o, oc = other.render_sensor_adaptive(d, ad)
            assert same_bytes(o, host) and np.array_equal(oc, counts)
    finally:
        other.close()


def test_errors(pkg, golden):
    hip = pkg.hip
    scene = golden("p10_s4_160x120").scene(pkg)
    out, counts = np.zeros((4, 8, 4), f32), np.zeros((4, 8), np.uint8)
    c = pkg.Context(0)
    try:
        h = c._h
        ok, ad = make(pkg, "equirect", 8, 4, 4), pkg.adaptive_defaults(min_samples=2)
        ref = lambda x: ctypes.byref(x) if x is not None else None

        def host(d, a, o=out.ctypes.data):
            rc = hip.rtu_render_sensor_adaptive(h, ref(d), ref(a), o, counts.ctypes.data)
            c.frame_status()  # clean afterwards
            return rc

        def device(d, a, o=8192):  # (every case below is refused before the pointer is written through)
            rc = hip.rtu_render_sensor_adaptive_device(h, ref(d), ref(a), o, None, None)
            c.frame_status()
            return rc
        assert host(ok, ad) == pkg.RTU_ERR_NO_SCENE and device(ok, ad) == pkg.RTU_ERR_NO_SCENE
        assert c.sensor_adaptive_trace() == []
        c.upload(scene)
        assert host(ok, ad) == pkg.RTU_OK
        assert hip.rtu_render_sensor_adaptive(h, ref(ok), ref(ad), out.ctypes.data, None) == pkg.RTU_OK  # counts may be NULL
        for what, d in refusals(pkg):
            assert host(d, ad) == pkg.RTU_ERR_ARG and device(d, ad) == pkg.RTU_ERR_ARG, what
        for s in (0, 256):
            d = make(pkg, "equirect", 8, 4, s)
            a = pkg.adaptive_defaults(min_samples=1)
            assert host(d, a) == pkg.RTU_ERR_ARG and device(d, a) == pkg.RTU_ERR_ARG, s
        for what, a in adaptive_violations(pkg, 4):
            assert host(ok, a) == pkg.RTU_ERR_ARG and device(ok, a) == pkg.RTU_ERR_ARG, what
        assert host(None, ad) == pkg.RTU_ERR_ARG and device(None, ad) == pkg.RTU_ERR_ARG
        assert host(ok, None) == pkg.RTU_ERR_ARG and device(ok, None) == pkg.RTU_ERR_ARG
        assert host(ok, ad, None) == pkg.RTU_ERR_ARG and device(ok, ad, None) == pkg.RTU_ERR_ARG and device(ok, ad, 8192 + 4) == pkg.RTU_ERR_ARG
        assert hip.rtu_debug_sensor_adaptive_trace(h, None, None, -1) == pkg.RTU_ERR_ARG
        # a raised cancel flag
        flag = ctypes.c_int(1)
        c.set_cancel(flag)
        assert host(ok, ad) == pkg.RTU_ERR_CANCELLED and device(ok, ad) == pkg.RTU_ERR_CANCELLED
        flag.value = 0
        good = out.copy()
        assert host(ok, ad) == pkg.RTU_OK and same_bytes(out, good)
        c.set_cancel(None)
        with pytest.raises(pkg.RtuError) as e:
            c.render_sensor_adaptive(make(pkg, "equirect", 8, 4, 0))
        assert e.value.code == pkg.RTU_ERR_ARG
    finally:
        c.close()
