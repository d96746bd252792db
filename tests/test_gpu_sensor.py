"""Sensors on the GPU (rtu_sensor_rays_device, rtu_render_sensor / _device; include/rtu_render.h, "Sensors").

The generator kernel is compared with the host specification byte for byte. The images are tied to what exists: recipe W to the ray-level
oracle under check_against of tests/test_gpu_parity.py (z bit for bit), the sampled recipes bit for bit in all four channels to the
numpy float32 sum, in sample order, of the existing host entries' answers to sensor_rays(desc, k), divided by n.
Sensor rays of recipes S and P, and the images made of them, meet the oracle in tests/test_gpu_rays_keyed.py (family K4)."""
import ctypes

import numpy as np
import pytest

from test_gpu_parity import check_against
from test_gpu_ray_query import lights
from test_gpu_workloads import GLASSROOM
from test_light_lists import RtuLight
from test_mesh_update_host import clone, deformed_scene
from test_sensor_host import BIG, camera_basis, make, refusals, valid

pytestmark = pytest.mark.gpu

f32 = np.float32
MODELS = ["equirect", "fisheye", "ortho"]


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def with_recipe(pkg, d, samples=0, gather_bounces=0, reference_walk=False):
    e = pkg.RtuSensorDesc.from_buffer_copy(bytes(d))
    e.samples, e.gather_bounces = samples, gather_bounces
    e.flags = pkg.RTU_QUERY_REFERENCE_WALK if reference_walk else 0
    return e


def mean_of_host_entries(pkg, ctx, d, per_sample=None):
    """The image by the rules of rtu_render.h from the existing host entries: shade_rays (recipe W), shade_rays_sampled (S) or
    shade_rays_paths (P) of sensor_rays(d, k), summed in sample order in float32, divided by n. per_sample(k, rays, out) sees each."""
    n = max(d.samples, 1)
    pixels = d.width * d.height
    s, zs, nh = np.zeros((pixels, 3), f32), np.zeros(pixels, f32), np.zeros(pixels, np.uint32)
    eye = tuple(d.pos)
    for k in range(n):
        rays, keys = pkg.sensor_rays(d, k)
        if d.samples == 0:
            out = ctx.shade_rays(rays, eye, max_bounce=d.max_bounce)[0]
        elif d.gather_bounces:
            out = ctx.shade_rays_paths(rays, keys, eye, max_bounce=d.max_bounce)[0]
        else:
            out = ctx.shade_rays_sampled(rays, keys, eye, max_bounce=d.max_bounce)[0]
        if per_sample:
            per_sample(k, rays, out)
        s += out[:, :3]
        hit = (out[:, 3] != BIG) & (out[:, 3] != 0)
        zs[hit] += out[hit, 3]
        nh[hit] += 1
    img = np.empty((pixels, 4), f32)
    img[:, :3] = s / f32(n)
    with np.errstate(all="ignore"):
        img[:, 3] = np.where(nh > 0, zs / nh.astype(f32), BIG)
    return img.reshape(d.height, d.width, 4)


def oracle_image(orc, scene, d, rays):
    """orc.shade_rays of the valid rays as an image; a ray that is not traced (outside the fisheye circle) is {0, 0, 0, RTU_BIGFLOAT}."""
    ok = valid(rays)
    img = np.zeros((rays.size, 4), f32)
    img[:, 3] = BIG
    img[ok] = orc.shade_rays(scene, np.ascontiguousarray(rays[ok]), eye=tuple(d.pos), threads=8, max_bounce=d.max_bounce)[0]
    return img.reshape(d.height, d.width, 4), ok.reshape(d.height, d.width)


# ---- 1. the generator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("size", [(1, 1), (37, 19), (65, 63)])
def test_generator_equals_the_host_form(pkg, model, size):
    import torch
    W, H = size
    pixels = W * H
    c = pkg.Context(0)  # no scene uploaded
    try:
        for samples, k0, nk in ((0, 0, 1), (5, 0, 1), (5, 2, 3)):
            d = make(pkg, model, W, H, samples, fov_deg=200.0)
            want = [pkg.sensor_rays(d, k) for k in range(k0, k0 + nk)]
            wrays = np.concatenate([np.ascontiguousarray(r).view(np.uint8).reshape(-1) for r, _ in want])
            wkeys = np.concatenate([q for _, q in want])
            n = pixels * nk
            for with_keys in (True, False):
                # 64 bytes of guard behind each buffer: nothing is written past the last ray
                d_rays = torch.full((n * 32 + 64,), 0x5A, dtype=torch.uint8, device="cuda:0")
                d_keys = torch.full((n + 16,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                c.sensor_rays_device(d, d_rays.data_ptr(), d_keys.data_ptr() if with_keys else None, k0, nk)
                torch.cuda.synchronize()
                got = d_rays.cpu().numpy()
                assert np.array_equal(got[:n * 32], wrays), "%s %dx%d samples [%d, %d) of %d" % (model, W, H, k0, k0 + nk, samples)
                assert (got[n * 32:] == 0x5A).all()
                gk = d_keys.cpu().numpy().view(np.uint32)
                assert np.array_equal(gk[:n], wkeys) if with_keys else (gk[:n] == 0x5A5A5A5A).all()
                assert (gk[n:] == 0x5A5A5A5A).all()
        c.frame_status()
        # a range of no samples is fine and writes nothing; a range outside the samples is refused
        d = make(pkg, model, W, H, 5)
        assert pkg.hip.rtu_sensor_rays_device(c._h, ctypes.byref(d), 5, 0, None, None, None) == pkg.RTU_OK
        for k0, nk in ((0, 6), (5, 1), (-1, 1), (0, -1)):
            assert pkg.hip.rtu_sensor_rays_device(c._h, ctypes.byref(d), k0, nk, 4096, None, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_sensor_rays_device(c._h, ctypes.byref(d), 0, 1, None, None, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_sensor_rays_device(c._h, ctypes.byref(d), 0, 1, 4096 + 8, None, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_sensor_rays_device(c._h, ctypes.byref(d), 0, 1, 4096, 8192 + 2, None) == pkg.RTU_ERR_ARG
    finally:
        c.close()


# ---- 2. recipe W against the oracle ----------------------------------------------------------------------------------------------
def scene_places(pkg, scene):
    """The camera's position and frame, a point inside the scene's box (a fifth of the way from its centre to the camera) and the
    box's diagonal."""
    pos, right, up, fwd = camera_basis(scene)
    box = pkg.scene_sort_box(scene).astype(np.float64)
    centre = 0.5 * (box[:3] + box[3:])
    inside = centre + 0.2 * (np.array(pos) - centre)
    assert (inside > box[:3]).all() and (inside < box[3:]).all()
    return {"camera": pos, "inside": tuple(float(f32(x)) for x in inside)}, (right, up, fwd), float(np.linalg.norm(box[3:] - box[:3]))


SENSORS = {"equirect": ("equirect", 96, 48, {}), "fisheye180": ("fisheye", 64, 64, dict(fov_deg=180.0)),
           "fisheye360": ("fisheye", 64, 64, dict(fov_deg=360.0)), "ortho": ("ortho", 64, 48, {})}


@pytest.mark.parametrize("tag", ["p4_240x135", "teapot2_240x135", "p7_200x150"])
@pytest.mark.parametrize("sensor", list(SENSORS))
def test_recipe_w_against_the_oracle(pkg, orc, ctx, golden, tag, sensor):
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    places, (right, up, fwd), diag = scene_places(pkg, scene)
    model, W, H, kw = SENSORS[sensor]
    for where, pos in places.items():
        d = pkg.sensor_desc(model, W, H, pos, right, up, fwd, extent=(diag, diag * H / W), **kw)
        rays, _ = pkg.sensor_rays(d)
        cpu, ok = oracle_image(orc, scene, d, rays)
        gpu = ctx.render_sensor(d)
        ctx.frame_status()
        hits = int((cpu[..., 3] != BIG).sum())
        print("%s %s from %s: %d of %d rays traced, %d hit" % (tag, sensor, where, int(ok.sum()), ok.size, hits))
        check_against(gpu, cpu, orc)
        assert np.array_equal(np.isnan(gpu[..., :3]), np.isnan(cpu[..., :3]))
        if model == "fisheye":
            assert not ok.all() and same_bytes(gpu[~ok], np.tile(np.array([0, 0, 0, BIG], f32), (int((~ok).sum()), 1)))
        else:
            assert ok.all()
        assert same_bytes(ctx.render_sensor(with_recipe(pkg, d, reference_walk=True)), gpu)
        assert same_bytes(gpu, mean_of_host_entries(pkg, ctx, d))


# ---- 3. the mean -------------------------------------------------------------------------------------------------------------------
MEAN_SCENES = {"p10_s4_160x120": 0, "p11gs_s2_160x90": 0, "p11_p2_120x68": 4, "p13_p2_96x72": 4, "p4_240x135": 0}  # tag -> gather_bounces


@pytest.mark.parametrize("tag", list(MEAN_SCENES))
@pytest.mark.parametrize("case", [("fisheye", 32, 32, 3), ("equirect", 40, 20, 5), ("ortho", 24, 12, 17)])  # 17: a batch of 16 and one of 1
def test_the_mean(pkg, orc, ctx, golden, tag, case):
    model, W, H, S = case
    scene = golden(tag).scene(pkg)
    ctx.upload(scene)
    places, (right, up, fwd), diag = scene_places(pkg, scene)
    d = pkg.sensor_desc(model, W, H, places["camera"], right, up, fwd, samples=S, gather_bounces=MEAN_SCENES[tag], fov_deg=200.0,
                        extent=(0.5 * diag, 0.25 * diag))
    seen = dict(hit=0, miss=0, invalid=0)

    def per_sample(k, rays, out):
        seen["hit"] += int(((out[:, 3] != BIG) & (out[:, 3] != 0)).sum())
        seen["miss"] += int((out[:, 3] == BIG).sum())
        seen["invalid"] += int((out[:, 3] == 0).sum())
        assert np.array_equal(out[:, 3] == 0, ~valid(rays))
        if tag == "p4_240x135":  # deterministic: recipe S draws nothing, and the oracle's Shade() is the bar
            cpu, _ = oracle_image(orc, scene, d, rays)
            img = out.reshape(H, W, 4).copy()
            img[out.reshape(H, W, 4)[..., 3] == 0, 3] = BIG
            check_against(img, cpu, orc)
    want = mean_of_host_entries(pkg, ctx, d, per_sample)
    got = ctx.render_sensor(d)
    ctx.frame_status()
    print("%s %s %dx%d, %d samples: %s" % (tag, model, W, H, S, seen))
    assert seen["hit"] > 0 and (model != "fisheye" or seen["invalid"] > 0)
    bad = int((got.view(np.uint32) != want.view(np.uint32)).any(axis=2).sum())
    assert bad == 0, "%d of %d pixels differ from the mean of the host entries" % (bad, W * H)


# ---- 4. sizes, and a capacity retry --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(1, 1), (63, 1), (64, 1), (65, 1), (37, 19)])
def test_sizes(pkg, ctx, golden, size):
    W, H = size
    scene = golden("teapot2_240x135").scene(pkg)
    ctx.upload(scene)
    places, (right, up, fwd), diag = scene_places(pkg, scene)
    for model in MODELS:
        for samples in (0, 2):
            d = pkg.sensor_desc(model, W, H, places["camera"], right, up, fwd, samples=samples, fov_deg=90.0, extent=(0.6 * diag, 0.3 * diag))
            assert same_bytes(ctx.render_sensor(d), mean_of_host_entries(pkg, ctx, d)), (model, size, samples)


def glassroom(pkg, tmp_path):
    """The glass room of tests/test_gpu_adaptive_oracle.py (its helper, copied): up to three child frames per ray, more frames than a
    fresh context provisions, made stochastic: glossy reflection, a point light with a size."""
    xml = GLASSROOM.replace('<reflection value="0.4"/>', '<reflection value="0.4" glossiness="0.05"/>')
    xml = xml.replace('<light type="point" name="p">', '<light type="point" name="p"><size value="2"/>')
    assert xml.count("glossiness=") == 1 and xml.count("<size") == 1
    path = tmp_path / "glassroom_soft.xml"
    path.write_text(xml)
    return pkg.Scene.from_xml(str(path))


def test_capacity_overflow_is_repaired(pkg, tmp_path):
    scene = glassroom(pkg, tmp_path)
    W, H = 128, 96
    # an orthographic window inside the ball's silhouette (radius 9): every ray hits the glass-and-mirror ball
    d = pkg.sensor_desc("ortho", W, H, (0.0, -14.0, 0.0), (1.0, 0.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), samples=2, extent=(12.0, 9.0))
    c = pkg.Context(0)  # a fresh context: nothing learned, nothing grown
    try:
        c.upload(scene)
        first = c.render_sensor(d)
        c.frame_status()  # clean: the render read and repaired the overflow itself
        frames, _ = c.frame_counts()
        assert max(frames[1:]) > 2 * W * H, frames  # more child frames in some level than the batch has rays: it did overflow
        second = c.render_sensor(d)
        c.frame_status()
        assert same_bytes(first, second)
        assert (first[..., 3] != BIG).all()
    finally:
        c.close()
    c2 = pkg.Context(0)
    try:
        c2.upload(scene)
        assert same_bytes(first, mean_of_host_entries(pkg, c2, d))
    finally:
        c2.close()


# ---- 5. it disturbs nothing ----------------------------------------------------------------------------------------------------------
def p10_sensor(pkg, scene, samples=3, W=48, H=24):
    pos, right, up, fwd = camera_basis(scene)
    return pkg.sensor_desc("equirect", W, H, pos, right, up, fwd, samples=samples)


def test_frames_and_sensors_leave_each_other_alone(pkg, golden):
    scene = golden("p10_s4_160x120").scene(pkg)
    c = pkg.Context(0)
    try:
        c.upload(scene)
        frame = pkg.frame_setup(scene.desc.camera, 96, 72, samples=3)
        d = p10_sensor(pkg, scene)
        before = c.render(frame)[0]
        img = c.render_sensor(d)
        assert same_bytes(c.render(frame)[0], before)
        a0 = None
        for k in range(5):
            assert same_bytes(c.render_sensor(d), img)
            assert same_bytes(c.render(frame)[0], before)
            if k == 0:
                a0 = pkg.hip.rtu_debug_device_allocations()
        assert pkg.hip.rtu_debug_device_allocations() == a0  # repeated sensor renders of one shape allocate nothing
    finally:
        c.close()


def test_an_open_progressive_session_is_not_disturbed(pkg, ctx, golden):
    scene = golden("p10_s4_160x120").scene(pkg)
    ctx.upload(scene)
    f = pkg.frame_setup(scene.desc.camera, 96, 72, samples=4)
    d = p10_sensor(pkg, scene)
    p = ctx.progressive(f)
    try:
        p.advance(2)
        snap0, _ = p.snapshot()
        img = ctx.render_sensor(d)
        snap1, _ = p.snapshot()
        assert same_bytes(snap0, snap1) and p.status()[0] == 2
        p.advance(2)
        assert same_bytes(p.snapshot()[0], ctx.render(f)[0])
        assert same_bytes(ctx.render_sensor(d), img)
    finally:
        p.close()


def test_sensors_follow_scene_updates(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    pos, right, up, fwd = camera_basis(scene)
    d = pkg.sensor_desc("fisheye", 48, 48, pos, right, up, fwd, fov_deg=60.0)

    def fresh(s):
        f = pkg.Context(0)
        try:
            f.upload(s)
            return f.render_sensor(d)
        finally:
            f.close()
    c = pkg.Context(0)
    try:
        c.upload(scene)
        out0 = c.render_sensor(d)
        relit = clone(pkg, scene)
        assert lights(relit)[1].type == 1  # the direct light: turned
        l = RtuLight.from_buffer_copy(bytes(lights(relit)[1]))
        l.vec[0], l.vec[1], l.vec[2] = l.vec[0] + 0.5, l.vec[1] - 0.25, l.vec[2]
        relit.set_light(1, l)
        c.update(relit)
        out1 = c.render_sensor(d)
        assert not same_bytes(out1, out0) and same_bytes(out1, fresh(relit))
        twisted = deformed_scene(pkg, relit, 0, ("twist", 120))
        c.update_meshes(twisted, [0])
        out2 = c.render_sensor(d)
        assert not same_bytes(out2, out1) and same_bytes(out2, fresh(twisted))
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
            d = pkg.sensor_desc("equirect", 40, 20, pos, right, up, fwd, samples=3, gather_bounces=gather)
            host = ctx.render_sensor(d)
            d_out = torch.full((40 * 20 * 4 + 16,), 7.0, dtype=torch.float32, device="cuda:0")
            torch.cuda.synchronize()
            ctx.render_sensor_device(d, d_out.data_ptr(), stream.cuda_stream)  # returns when the image is complete
            ctx.frame_status()
            dev = d_out.cpu().numpy()
            assert same_bytes(dev[:-16].reshape(20, 40, 4), host) and (dev[-16:] == 7.0).all()
            assert same_bytes(other.render_sensor(d), host)
            # the kernel timing diagnostic changes no byte and reports the two kernels inside the render
            ctx.sensor_timing(True)
            assert same_bytes(ctx.render_sensor(d), host)
            t = ctx.sensor_timing(False)
            assert t["rays"] > 0 and t["accumulate"] > 0 and t["render"] >= t["rays"] + t["accumulate"]
            assert same_bytes(ctx.render_sensor(d), host) and ctx.sensor_timing(False) == dict(rays=0.0, accumulate=0.0, render=0.0)
    finally:
        other.close()


# ---- 6. errors ---------------------------------------------------------------------------------------------------------------------
def test_errors(pkg, golden):
    hip = pkg.hip
    scene = golden("p10_s4_160x120").scene(pkg)
    plain = golden("p4_240x135").scene(pkg)
    out = np.zeros((4, 8, 4), f32)
    c = pkg.Context(0)
    try:
        h = c._h
        ok = make(pkg, "equirect", 8, 4, 2)

        def host(d, o=out.ctypes.data):
            rc = hip.rtu_render_sensor(h, ctypes.byref(d) if d is not None else None, o)
            c.frame_status()  # clean afterwards
            return rc

        def device(d, o=8192):  # (every case below is refused before the pointer is written through)
            rc = hip.rtu_render_sensor_device(h, ctypes.byref(d) if d is not None else None, o, None)
            c.frame_status()
            return rc
        assert host(ok) == pkg.RTU_ERR_NO_SCENE and device(ok) == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        assert host(ok) == pkg.RTU_OK
        for what, d in refusals(pkg):
            assert host(d) == pkg.RTU_ERR_ARG and device(d) == pkg.RTU_ERR_ARG, what
        assert host(None) == pkg.RTU_ERR_ARG and device(None) == pkg.RTU_ERR_ARG
        assert host(ok, None) == pkg.RTU_ERR_ARG and device(ok, None) == pkg.RTU_ERR_ARG and device(ok, 8192 + 4) == pkg.RTU_ERR_ARG
        # recipe W refuses a stochastic scene, as rtu_shade_rays does
        w = make(pkg, "equirect", 8, 4, 0)
        assert host(w) == pkg.RTU_ERR_STOCHASTIC and device(w) == pkg.RTU_ERR_STOCHASTIC
        with pytest.raises(pkg.RtuError) as e:
            c.render_sensor(w)
        assert e.value.code == pkg.RTU_ERR_STOCHASTIC
        # a raised cancel flag
        flag = ctypes.c_int(1)
        c.set_cancel(flag)
        assert host(ok) == pkg.RTU_ERR_CANCELLED and device(ok) == pkg.RTU_ERR_CANCELLED
        flag.value = 0
        good = out.copy()
        assert host(ok) == pkg.RTU_OK and same_bytes(out, good)
        c.set_cancel(None)
        c.upload(plain)
        assert host(w) == pkg.RTU_OK
    finally:
        c.close()
