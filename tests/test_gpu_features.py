"""First-hit features (rtu_ray_features / rtu_frame_features, include/rtu_render.h) against the entries that already compute their
two halves: the hit is rtu_trace_rays', byte for byte; the albedo is Shade() with bounceCount 0 under one ambient light of
intensity 1 — the rgb of rtu_shade_rays on a context holding the all-ambient clone of the scene, bit for bit, and the oracle's
shade of that clone under the bar of tests/test_gpu_shade_rays.py."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import ambient_clone
from test_gpu_ray_query import bits, frame_of, materials, same_hits
from test_gpu_shade_rays import against_oracle
from test_mesh_update_host import clone

pytestmark = pytest.mark.gpu

F = np.float32
BIG = F(1.0e30)
TAGS = ["teapot2_240x135", "p7_200x150", "mtl_160x120", "p4_240x135", "p13_200x150"]  # 90 % misses; textures; MultiMtl; spheres; a box room
RTU_RAY_HIT, RTU_RAY_FRONT, RTU_RAY_INVALID = 1, 2, 4
RTU_ERR_STOCHASTIC = -4


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def mixed_rays(pkg, orc, scene, frame, seed):
    """The camera rays of `frame`, some 600 rays that continue behind the camera rays' hits (they leave the objects through back
    faces) and some 300 invalid or mis-normalised rays, shuffled: (rays, valid mask)."""
    rng = np.random.default_rng(seed)
    cam = pkg.camera_rays(frame)
    h = orc.trace_rays(scene, cam, threads=8)
    hi = np.flatnonzero((h["flags"] & RTU_RAY_HIT) != 0)
    hi = hi[::max(1, len(hi) // 600)]
    cont = np.zeros(len(hi), pkg.ray_dtype())
    cont["org"] = h["p"][hi] + cam["dir"][hi] * F(0.01)
    cont["dir"], cont["tmax"] = cam["dir"][hi], BIG
    bad = cam[rng.integers(0, cam.size, 300)].copy()
    kind = np.arange(300) % 6
    bad["org"][kind == 0, 1] = np.nan
    bad["dir"][kind == 1, 0] = np.inf
    bad["tmax"][kind == 2] = F(0.0)
    bad["dir"][kind == 3] *= F(1.1)
    bad["dir"][kind == 4] = 0.0
    bad["dir"][kind == 5] *= F(0.9)
    rays = np.concatenate([cam, cont, bad])
    valid = np.concatenate([np.ones(cam.size + cont.size, bool), np.zeros(300, bool)])
    order = rng.permutation(rays.size)
    return np.ascontiguousarray(rays[order]), valid[order]


def ambient_shade(pkg, c, rays, eye):
    """rtu_shade_rays with max_bounce 0 on the context `c` (which holds an all-ambient clone); a scene recipe W refuses as
    stochastic goes through rtu_shade_rays_sampled with arbitrary keys (no light is left to sample, max_bounce 0 bounces nothing)."""
    try:
        return c.shade_rays(rays, eye, max_bounce=0)[0]
    except pkg.RtuError as e:
        if e.code != RTU_ERR_STOCHASTIC:
            raise
        return c.shade_rays_sampled(rays, np.arange(rays.size, dtype=np.uint32) * np.uint32(2654435761), eye, max_bounce=0)[0]


# ---- 4. the ray form against the existing entries -----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_ray_features_against_trace_rays_shade_rays_and_the_oracle(pkg, orc, golden, ctx, tag):
    g = golden(tag)
    scene = g.scene(pkg)
    frame = frame_of(pkg, scene, g.width, g.height)
    eye = tuple(frame.cam_pos)
    rays, valid = mixed_rays(pkg, orc, scene, frame, 99)
    ctx.upload(scene)
    want_hits = ctx.trace_rays(rays)
    hits, albedo = ctx.ray_features(rays)
    assert same_hits(hits, want_hits)
    hits_ref, albedo_ref = ctx.ray_features(rays, reference_walk=True)
    assert same_hits(hits_ref, want_hits) and np.array_equal(bits(albedo_ref), bits(albedo))
    hit = (hits["flags"] & RTU_RAY_HIT) != 0
    front = (hits["flags"] & RTU_RAY_FRONT) != 0
    assert (hits["flags"][~valid] == RTU_RAY_INVALID).all() and not hit[~valid].any()
    assert not bits(albedo)[~hit].any(), "albedo at a miss or an invalid ray is four zeros"
    assert not bits(albedo[:, 3]).any()
    # what the existing entries shade with one ambient light of intensity 1
    amb = ambient_clone(pkg, scene)
    other = pkg.Context(0)
    try:
        other.upload(amb)
        shaded = ambient_shade(pkg, other, rays, eye)
    finally:
        other.close()
    assert np.array_equal(bits(albedo[hit, :3]), bits(shaded[hit, :3])), "albedo differs from rtu_shade_rays of the all-ambient clone"
    assert np.array_equal(bits(hits["t"][valid]), bits(shaded[valid, 3]))
    # the oracle's Shade() of the clone, valid rays only (its ray entry filters nothing)
    cpu = orc.shade_rays(amb, rays[valid], eye=eye, threads=8, max_bounce=0)[0]
    out = np.concatenate([albedo[valid, :3], hits["t"][valid, None]], axis=1)
    ohit = against_oracle(out, cpu, orc)
    assert np.array_equal(ohit, hit[valid])
    ndiff = int((bits(out[ohit, :3]) != bits(cpu[ohit, :3])).sum())
    print("%s: %d rays, %d hits, %d back faces; albedo words that differ from the oracle's: %d" %
          (tag, rays.size, hit.sum(), (hit & ~front).sum(), ndiff))
    # non-vacuity
    assert (hit & ~front).any(), "no back-face hit"
    assert not albedo[hit & ~front & (hits["material"] >= 0), :3].any(), "a back face is black"
    assert (hit & front).sum() > 1000 and albedo[hit & front, :3].any()
    mats = materials(scene)
    flat = np.array([list(mats[int(m)].diffuse) if m >= 0 else [1.0, 1.0, 1.0] for m in hits["material"][hit & front]], F)
    textured = (bits(flat) != bits(albedo[hit & front, :3])).any(axis=1)
    if tag in ("p7_200x150", "mtl_160x120"):
        assert scene.desc.material_maps and textured.sum() > 100, "no textured hit"
    else:
        assert not textured.any()
    if tag == "mtl_160x120":
        assert len(np.unique(hits["material"][hit])) >= 2, "one sub-material only"
    if tag == "teapot2_240x135":
        assert (~hit[valid]).mean() > 0.8


def test_batch_sizes_and_the_device_form(pkg, golden, ctx):
    import torch
    g = golden("p7_200x150")
    scene = g.scene(pkg)
    ctx.upload(scene)
    rays = pkg.camera_rays(frame_of(pkg, scene, g.width, g.height))
    hits, albedo = ctx.ray_features(rays)
    step = rays.size // 65
    for n in (0, 1, 63, 64, 65):
        h, a = ctx.ray_features(rays[::step][:n])
        assert h.size == n and same_hits(h, hits[::step][:n]) and np.array_equal(bits(a), bits(albedo[::step][:n]))
    stream = torch.cuda.Stream(device=0)
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to("cuda:0")
    d_hits = torch.zeros(rays.size * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.full((rays.size, 4), 7.0, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    a0 = pkg.hip.rtu_debug_device_allocations()
    for ref in (False, True):
        ctx.ray_features_device(d_rays.data_ptr(), rays.size, d_hits.data_ptr(), d_alb.data_ptr(), stream.cuda_stream, reference_walk=ref)
        stream.synchronize()
        assert same_hits(d_hits.cpu().numpy().view(pkg.hit_dtype()), hits) and np.array_equal(bits(d_alb.cpu().numpy()), bits(albedo))
    assert pkg.hip.rtu_debug_device_allocations() == a0


# ---- 5. the frame form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_frame_features_equal_ray_features_of_the_camera_rays(pkg, golden, ctx, tag):
    import torch
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    for W, H in ((g.width, g.height), (67, 35)):
        frame = frame_of(pkg, scene, W, H)
        want_hits, want_albedo = ctx.ray_features(pkg.camera_rays(frame))
        hits, albedo = ctx.frame_features(frame)
        assert same_hits(hits, want_hits) and np.array_equal(bits(albedo), bits(want_albedo))
        # samples, gather_bounces and max_bounce are ignored; the device form writes the same bytes
        sampled = pkg.frame_setup(scene.desc.camera, W, H, samples=4, gather_bounces=4, max_bounce=2)
        d_hits = torch.zeros(W * H * 48, dtype=torch.uint8, device="cuda:0")
        d_alb = torch.full((W * H, 4), 7.0, dtype=torch.float32, device="cuda:0")
        ctx.frame_features_device(sampled, d_hits.data_ptr(), d_alb.data_ptr())
        torch.cuda.synchronize()
        assert same_hits(d_hits.cpu().numpy().view(pkg.hit_dtype()), want_hits) and np.array_equal(bits(d_alb.cpu().numpy()), bits(want_albedo))
    sharded = pkg.frame_setup(scene.desc.camera, g.width, g.height, shard_rank=1, shard_count=2)
    with pytest.raises(pkg.RtuError) as e:
        ctx.frame_features(sharded)
    assert e.value.code == pkg.RTU_ERR_ARG
    with pytest.raises(pkg.RtuError) as e:
        ctx.frame_features_device(sharded, 16, 16)
    assert e.value.code == pkg.RTU_ERR_ARG


# ---- 6. scene updates ----------------------------------------------------------------------------------------------------------------
def test_albedo_follows_scene_updates(pkg, golden):
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    frame = frame_of(pkg, scene, g.width, g.height)
    c = pkg.Context(0)
    try:
        c.upload(scene)
        h0, a0 = c.frame_features(frame)
        front = (h0["flags"] & (RTU_RAY_HIT | RTU_RAY_FRONT)) == (RTU_RAY_HIT | RTU_RAY_FRONT)
        m = int(np.bincount(h0["material"][front]).argmax())
        mine = front & (h0["material"] == m)
        assert mine.sum() > 500 and (front & ~mine).any()
        painted = clone(pkg, scene)
        new = (F(0.125), F(0.7), F(0.3))
        for k in range(3):
            materials(painted)[m].diffuse[k] = new[k]
        assert not np.array_equal(a0[mine][0, :3], np.array(new, F))
        c.update(painted)
        h1, a1 = c.frame_features(frame)
        assert same_hits(h0, h1)
        assert np.array_equal(bits(a1[mine, :3]), bits(np.tile(np.array(new, F), (mine.sum(), 1))))
        assert np.array_equal(bits(a1[~mine]), bits(a0[~mine]))
    finally:
        c.close()


def test_errors(pkg, golden):
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    frame = frame_of(pkg, scene, g.width, g.height)
    rays = np.ascontiguousarray(pkg.camera_rays(frame)[:8])
    hits, alb = np.zeros(8, pkg.hit_dtype()), np.zeros((8, 4), F)
    fh, fa = np.zeros(frame.width * frame.height, pkg.hit_dtype()), np.zeros((frame.width * frame.height, 4), F)
    c = pkg.Context(0)
    hip = pkg.hip
    try:
        assert hip.rtu_ray_features(c._h, rays.ctypes.data, 8, 0, hits.ctypes.data, alb.ctypes.data) == pkg.RTU_ERR_NO_SCENE
        assert hip.rtu_ray_features_device(c._h, 16, 8, 0, 16, 16, None) == pkg.RTU_ERR_NO_SCENE  # (refused before any pointer is read)
        assert hip.rtu_frame_features(c._h, ctypes.byref(frame), fh.ctypes.data, fa.ctypes.data) == pkg.RTU_ERR_NO_SCENE
        assert hip.rtu_frame_features_device(c._h, ctypes.byref(frame), 16, 16, None) == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        assert hip.rtu_ray_features(c._h, rays.ctypes.data, 8, 0, hits.ctypes.data, alb.ctypes.data) == pkg.RTU_OK
        for flags in (2, 4, 0x80000000, 3):
            assert hip.rtu_ray_features(c._h, rays.ctypes.data, 8, flags, hits.ctypes.data, alb.ctypes.data) == pkg.RTU_ERR_ARG
            assert hip.rtu_ray_features_device(c._h, 16, 8, flags, 16, 16, None) == pkg.RTU_ERR_ARG
        for k in range(3):
            args = [rays.ctypes.data, hits.ctypes.data, alb.ctypes.data]
            args[k] = None
            assert hip.rtu_ray_features(c._h, args[0], 8, 0, args[1], args[2]) == pkg.RTU_ERR_ARG
            dev = [16, 16, 16]
            dev[k] = None
            assert hip.rtu_ray_features_device(c._h, dev[0], 8, 0, dev[1], dev[2], None) == pkg.RTU_ERR_ARG
            dev[k] = 24  # not 16-byte aligned
            assert hip.rtu_ray_features_device(c._h, dev[0], 8, 0, dev[1], dev[2], None) == pkg.RTU_ERR_ARG
        assert hip.rtu_ray_features(c._h, None, 0, 0, None, None) == pkg.RTU_OK            # n == 0 launches nothing
        assert hip.rtu_ray_features_device(c._h, None, 0, 0, None, None, None) == pkg.RTU_OK
        assert hip.rtu_ray_features(None, rays.ctypes.data, 8, 0, hits.ctypes.data, alb.ctypes.data) == pkg.RTU_ERR_ARG
        assert hip.rtu_frame_features(c._h, None, fh.ctypes.data, fa.ctypes.data) == pkg.RTU_ERR_ARG
        assert hip.rtu_frame_features(c._h, ctypes.byref(frame), None, fa.ctypes.data) == pkg.RTU_ERR_ARG
        assert hip.rtu_frame_features(c._h, ctypes.byref(frame), fh.ctypes.data, None) == pkg.RTU_ERR_ARG
        assert hip.rtu_frame_features_device(c._h, ctypes.byref(frame), 24, 16, None) == pkg.RTU_ERR_ARG
        assert hip.rtu_frame_features_device(c._h, ctypes.byref(frame), 16, 8, None) == pkg.RTU_ERR_ARG
        assert hip.rtu_frame_features_device(c._h, ctypes.byref(frame), None, 16, None) == pkg.RTU_ERR_ARG
        empty = pkg.frame_setup(scene.desc.camera, g.width, g.height)
        empty.width = 0
        assert hip.rtu_frame_features(c._h, ctypes.byref(empty), fh.ctypes.data, fa.ctypes.data) == pkg.RTU_ERR_ARG
    finally:
        c.close()
