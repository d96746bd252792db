"""The two halves of a recipe-P sample (rtu_gather_rays / rtu_shade_rays_ambient, include/rtu_render.h) against the entries the oracle
already checks: rtu_shade_rays_paths, which computes and consumes the gathered AmbientLight in one go, and rtu_shade_rays_sampled,
which has none. Scenes: the recipe-P goldens p11_p2_120x68 and p13_p2_96x72; rays and keys: rtu_camera_sample_rays(frame, k) for two k."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

from test_gpu_ray_query import BIG, materials
from test_gpu_shade_rays_sampled import eye_of, same_bytes

pytestmark = pytest.mark.gpu

TAGS = ["p11_p2_120x68", "p13_p2_96x72"]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cam(pkg, golden, ctx):
    """Per golden tag, computed once and left unchanged: per sample the rays, keys, and what the three host entries give them."""
    cache = {}

    def get(tag):
        if tag not in cache:
            g = golden(tag)
            scene = g.scene(pkg)
            ctx.upload(scene)
            frame = pkg.frame_setup(scene.desc.camera, g.width, g.height, samples=2, gather_bounces=4)
            eye = eye_of(frame)
            s = SimpleNamespace(scene=scene, frame=frame, eye=eye, rays=[], keys=[], paths=[], sampled=[], gather=[])
            for k in range(2):
                r, q = pkg.camera_sample_rays(frame, k)
                arrays = (r, q, ctx.shade_rays_paths(r, q, eye)[0], ctx.shade_rays_sampled(r, q, eye)[0], ctx.gather_rays(r, q, eye)[0])
                for a, dst in zip(arrays, (s.rays, s.keys, s.paths, s.sampled, s.gather)):
                    a.setflags(write=False)
                    dst.append(a)
            cache[tag] = s
        return cache[tag]
    return get


@pytest.mark.parametrize("tag", TAGS)
def test_the_two_halves_make_the_path_traced_batch(pkg, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    for k in range(2):
        both = ctx.shade_rays_ambient(c.rays[k], c.keys[k], c.gather[k], c.eye)[0]
        assert same_bytes(both, c.paths[k]), "sample %d: ambient(gather) is not the path-traced batch" % k
        assert same_bytes(c.gather[k][:, 3], c.paths[k][:, 3])  # t follows rtu_shade_rays_paths
        lit = int((c.gather[k][:, :3] > 0).any(axis=1).sum())
        print("%s sample %d: %d rays, %d hit, %d with a gathered light" % (tag, k, len(both), int((both[:, 3] < BIG).sum()), lit))
        assert lit > len(both) // 2  # the gather is really there
        # a three-column amb is the same call
        assert same_bytes(ctx.shade_rays_ambient(c.rays[k][:500], c.keys[k][:500], c.gather[k][:500, :3], c.eye)[0], c.paths[k][:500])


@pytest.mark.parametrize("tag", TAGS)
def test_without_ambient_light_it_is_the_sampled_batch(pkg, ctx, cam, tag):
    c = cam(tag)
    ctx.upload(c.scene)
    for k in range(2):
        none = ctx.shade_rays_ambient(c.rays[k], c.keys[k], np.zeros((c.rays[k].size, 4), np.float32), c.eye)[0]
        assert same_bytes(none, c.sampled[k])
        # the fourth float of amb is ignored
        amb = np.zeros((c.rays[k].size, 4), np.float32)
        amb[:, 3] = 123.0
        assert same_bytes(ctx.shade_rays_ambient(c.rays[k], c.keys[k], amb, c.eye)[0], c.sampled[k])


@pytest.mark.parametrize("tag", TAGS)
def test_diffuse_times_c_is_paths_minus_sampled(pkg, ctx, cam, tag):
    """At a front-face hit of a material without reflection, refraction or a diffuse map the ambient tree is `diffuse * c` and nothing
    else (mtlFunctions.cpp:125-132), so paths = fl(fl(0 + fl(diffuse * c)) + sampled) per channel. Three roundings to binary32, each at
    most max(2^-24 |x|, 2^-150) away from its exact value x (half a unit in the last place; 2^-150 is half the spacing of the
    subnormals, where the relative bound no longer holds — a gathered c of 7e-44 occurs on p13): the product, x = diffuse * c; the sum
    with zero, exact; the final sum, |x| <= |paths| (1 + 2^-24). paths - sampled and diffuse * c are both exact in binary64 (a difference
    and a product of binary32 numbers), so
        |(paths - sampled) - diffuse * c| <= 2^-24 (|paths| + |diffuse * c|) + 2 * 2^-150."""
    c = cam(tag)
    ctx.upload(c.scene)
    mats = materials(c.scene)
    n_mat = c.scene.desc.n_materials
    childless = np.array([not any(mats[m].reflection) and not any(mats[m].refraction) for m in range(n_mat)])
    mapped = np.zeros(n_mat, bool)
    if c.scene.desc.n_textures and c.scene.desc.material_maps:
        maps = ctypes.cast(c.scene.desc.material_maps, ctypes.POINTER(pkg.RtuTexMap))
        mapped = np.array([bool(maps[4 * m].present) for m in range(n_mat)])  # (4 * material + RTU_MAP_DIFFUSE)
    diffuse = np.array([list(mats[m].diffuse) for m in range(n_mat)], np.float32)
    checked = 0
    for k in range(2):
        hits = ctx.trace_rays(c.rays[k])
        mid = hits["material"]
        ok = ((hits["flags"] & pkg.RTU_RAY_HIT) != 0) & ((hits["flags"] & pkg.RTU_RAY_FRONT) != 0) & (mid >= 0)
        ok[ok] &= childless[mid[ok]] & ~mapped[mid[ok]]
        want = diffuse[mid[ok]].astype(np.float64) * c.gather[k][ok, :3].astype(np.float64)
        got = c.paths[k][ok, :3].astype(np.float64) - c.sampled[k][ok, :3].astype(np.float64)
        bound = 2.0 ** -24 * (np.abs(c.paths[k][ok, :3].astype(np.float64)) + np.abs(want)) + 2.0 * 2.0 ** -150
        err = np.abs(got - want)
        print("%s sample %d: %d front-face hits of childless materials; largest error %.3g, largest error / bound %.3g"
              % (tag, k, int(ok.sum()), err.max(), (err / bound).max()))
        assert np.all(err <= bound)
        checked += int(ok.sum())
    assert checked > 1000


def device_buffers(rays, keys, amb=None, fill=7.0):
    import torch
    d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to("cuda:0")
    d_keys = torch.from_numpy(np.ascontiguousarray(keys).view(np.int32).copy()).to("cuda:0")
    d_amb = torch.from_numpy(np.ascontiguousarray(amb, np.float32).copy()).to("cuda:0") if amb is not None else None
    d_out = torch.full((rays.size * 4,), fill, dtype=torch.float32, device="cuda:0")
    torch.cuda.synchronize()
    return d_rays, d_keys, d_amb, d_out


def until_it_fits(pkg, ctx, call):
    for attempt in range(8):
        call()
        try:
            ctx.frame_status()
            return
        except pkg.RtuError as err:
            assert err.code == pkg.RTU_ERR_CAPACITY
    raise AssertionError("capacity never sufficed")


@pytest.mark.parametrize("tag", TAGS)
def test_device_forms_and_the_reference_walk(pkg, ctx, cam, tag):
    import torch
    c = cam(tag)
    ctx.upload(c.scene)
    k = 1
    stream = torch.cuda.Stream(device=0)
    refs = (False, True)
    for ref in refs:
        rays, keys, gather, paths = c.rays[k], c.keys[k], c.gather[k], c.paths[k]
        d_rays, d_keys, d_amb, d_out = device_buffers(rays, keys, gather)
        until_it_fits(pkg, ctx, lambda: ctx.gather_rays_device(d_rays.data_ptr(), d_keys.data_ptr(), rays.size, c.eye, d_out.data_ptr(), stream.cuda_stream,
                                                               reference_walk=ref))
        assert same_bytes(d_out.cpu().numpy().reshape(-1, 4), gather)
        d_out.fill_(7.0)
        torch.cuda.synchronize()
        until_it_fits(pkg, ctx, lambda: ctx.shade_rays_ambient_device(d_rays.data_ptr(), d_keys.data_ptr(), d_amb.data_ptr(), rays.size, c.eye, d_out.data_ptr(),
                                                                      stream.cuda_stream, reference_walk=ref))
        assert same_bytes(d_out.cpu().numpy().reshape(-1, 4), paths)
        d_out.fill_(7.0)
        torch.cuda.synchronize()
    # the host forms' counting variant: the same bytes, and the roots are counted
    g_ref, st = ctx.gather_rays(rays, keys, c.eye, reference_walk=True, stats=True)
    assert same_bytes(g_ref, gather) and st["primary_rays"] == rays.size
    a_ref, st = ctx.shade_rays_ambient(rays, keys, gather, c.eye, stats=True)
    assert same_bytes(a_ref, paths) and st["primary_rays"] == rays.size


def test_misses_invalid_rays_and_order(pkg, ctx, cam):
    """Rays that leave the scene, an invalid ray, and a shuffled batch: c = 0 and the t of rtu_shade_rays_paths where nothing is
    shaded; the answer to a ray depends on the ray and its key, not on its place."""
    c = cam("p13_p2_96x72")
    ctx.upload(c.scene)
    rays, keys = c.rays[0][:4096].copy(), c.keys[0][:4096].copy()
    rays["dir"][::7] *= -1.0       # away from the scene (some still hit the room behind the camera)
    rays["dir"][5] = 0.0           # invalid: not of unit length
    rays["tmax"][9] = 1e-3         # too short to hit anything: a miss with t = tmax
    paths = ctx.shade_rays_paths(rays, keys, c.eye)[0]
    gather = ctx.gather_rays(rays, keys, c.eye)[0]
    assert same_bytes(gather[:, 3], paths[:, 3])
    assert same_bytes(gather[5], np.zeros(4, np.float32))
    assert gather[9, 3] == np.float32(1e-3) and not gather[9, :3].any()
    hits = ctx.trace_rays(rays)
    miss = (hits["flags"] & pkg.RTU_RAY_HIT) == 0
    assert miss.sum() >= 2 and not gather[miss, :3].any()
    assert same_bytes(ctx.shade_rays_ambient(rays, keys, gather, c.eye)[0], paths)
    perm = np.random.default_rng(3).permutation(rays.size)
    assert same_bytes(ctx.gather_rays(rays[perm], keys[perm], c.eye)[0], gather[perm])
    assert same_bytes(ctx.shade_rays_ambient(rays[perm], keys[perm], gather[perm], c.eye)[0], paths[perm])


def test_errors(pkg, cam):
    c = cam("p11_p2_120x68")
    hip = pkg.hip
    r = np.ascontiguousarray(c.rays[0][:8])
    q = np.ascontiguousarray(c.keys[0][:8])
    a = np.ascontiguousarray(c.gather[0][:8])
    out = np.zeros((8, 4), np.float32)
    ctx = pkg.Context(0)
    try:
        h = ctx._h
        ok = pkg.shade_desc(c.eye)

        def gather(desc, rays=r.ctypes.data, keys=q.ctypes.data, o=out.ctypes.data, n=8):
            return hip.rtu_gather_rays(h, rays, keys, n, ctypes.byref(desc) if desc is not None else None, o, None)

        def ambient(desc, rays=r.ctypes.data, keys=q.ctypes.data, amb=a.ctypes.data, o=out.ctypes.data, n=8):
            return hip.rtu_shade_rays_ambient(h, rays, keys, amb, n, ctypes.byref(desc) if desc is not None else None, o, None)

        def gather_d(desc, rays=4096, keys=16384, o=8192, n=8):  # (every case below is refused before a pointer is read)
            return hip.rtu_gather_rays_device(h, rays, keys, n, ctypes.byref(desc) if desc is not None else None, o, None)

        def ambient_d(desc, rays=4096, keys=16384, amb=32768, o=8192, n=8):
            return hip.rtu_shade_rays_ambient_device(h, rays, keys, amb, n, ctypes.byref(desc) if desc is not None else None, o, None)
        for f in (gather, ambient, gather_d, ambient_d):
            assert f(ok) == pkg.RTU_ERR_NO_SCENE
        ctx.upload(c.scene)
        assert gather(ok) == pkg.RTU_OK and same_bytes(out, c.gather[0][:8])
        assert ambient(ok) == pkg.RTU_OK and same_bytes(out, c.paths[0][:8])
        # n == 0: fine, whatever the pointers, and nothing is launched
        counts = ctx.frame_counts()
        assert gather(ok, None, None, None, 0) == pkg.RTU_OK and ambient(ok, None, None, None, None, 0) == pkg.RTU_OK
        assert gather_d(ok, None, None, None, 0) == pkg.RTU_OK and ambient_d(ok, None, None, None, None, 0) == pkg.RTU_OK
        assert ctx.frame_counts() == counts
        for f in (gather, ambient, gather_d, ambient_d):
            assert f(None) == pkg.RTU_ERR_ARG
            assert f(ok, rays=None) == pkg.RTU_ERR_ARG and f(ok, keys=None) == pkg.RTU_ERR_ARG and f(ok, o=None) == pkg.RTU_ERR_ARG
        assert ambient(ok, amb=None) == pkg.RTU_ERR_ARG and ambient_d(ok, amb=None) == pkg.RTU_ERR_ARG
        assert ambient_d(ok, amb=32768 + 4) == pkg.RTU_ERR_ARG and ambient(ok, amb=a.ctypes.data + 2) == pkg.RTU_ERR_ARG
        assert gather_d(ok, rays=4096 + 8) == pkg.RTU_ERR_ARG and gather_d(ok, o=8192 + 4) == pkg.RTU_ERR_ARG and gather_d(ok, keys=16384 + 2) == pkg.RTU_ERR_ARG
        assert gather_d(ok, n=(1 << 25) + 1) == pkg.RTU_ERR_ARG and ambient_d(ok, n=(1 << 25) + 1) == pkg.RTU_ERR_ARG
        for flags in (2, 0x80000000):
            d = pkg.shade_desc(c.eye)
            d.flags = flags
            assert gather(d) == pkg.RTU_ERR_ARG and ambient_d(d) == pkg.RTU_ERR_ARG
        d = pkg.shade_desc(c.eye)
        d.reserved[1] = 1
        assert gather_d(d) == pkg.RTU_ERR_ARG and ambient(d) == pkg.RTU_ERR_ARG
        for mb in (-1, 6):
            d = pkg.shade_desc(c.eye)
            d.max_bounce = mb
            assert gather(d) == pkg.RTU_ERR_ARG and ambient(d) == pkg.RTU_ERR_ARG
        d = pkg.shade_desc(c.eye)
        d.eye[1] = float("inf")
        assert gather(d) == pkg.RTU_ERR_ARG and ambient_d(d) == pkg.RTU_ERR_ARG
        assert hip.rtu_gather_rays(None, r.ctypes.data, q.ctypes.data, 8, ctypes.byref(ok), out.ctypes.data, None) == pkg.RTU_ERR_ARG
        ctx.frame_status()
        # the context still works
        assert gather(ok) == pkg.RTU_OK and same_bytes(out, c.gather[0][:8])
    finally:
        ctx.close()
