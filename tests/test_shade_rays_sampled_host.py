"""Sampled ray batches (rtu_shade_rays_sampled, include/rtu_render.h), the part that needs no GPU: the five symbols, the two key
functions against the header's formulas, rtu_camera_sample_rays against a numpy binary32 restatement of primary_pixel's recipe-S
branch — rays and keys bit for bit —, its refusals and the NULL-context answers."""
import ctypes

import numpy as np
import pytest

from test_mesh_update_host import clone

U32 = np.uint32


def u32(x):
    return np.atleast_1d(np.asarray(x, U32))  # (arrays wrap silently where numpy's scalars warn)


def mix32(x):
    x = u32(x).copy()
    x ^= x >> U32(16)
    x *= U32(0x7feb352d)
    x ^= x >> U32(15)
    x *= U32(0x846ca68b)
    x ^= x >> U32(16)
    return x


def np_sample_key(p, i):
    return mix32(mix32(u32(p) + U32(0x68bc21eb)) ^ (u32(i) * U32(0x9e3779b9) + U32(1)))


def np_child_key(key, slot):
    return mix32(u32(key) + (u32(slot) + U32(1)) * U32(0x632be5ab))


def np_rand31(key, purpose):
    return mix32(u32(key) ^ mix32(u32(purpose) * U32(0x9e3779b9) + U32(0x85ebca6b))) >> U32(1)


def halton(index, base):
    """scene.h:130-139 in binary32."""
    f32 = np.float32
    r, f, i = f32(0), f32(1) / f32(base), index
    while i > 0:
        r = f32(r + f32(f * f32(i % base)))
        f = f32(f / f32(base))
        i //= base
    return r


def numpy_sample_rays(orc, frame, sample, row0, nrows):
    """primary_pixel's recipe-S branch (RenderFunctions.cpp:80-97, :258-268) in numpy binary32, the lens angle through the oracle's
    portable_sincos: (rays [nrows * W, 8] float32 with reserved 0, keys)."""
    f32 = np.float32
    W, S = frame.width, frame.samples
    v3 = lambda a: np.array(list(a), f32)
    pos, origin, u, v, up, right = (v3(a) for a in (frame.cam_pos, frame.origin, frame.u, frame.v, frame.lens_up, frame.lens_right))
    dof = f32(frame.dof)
    inc = f32(1.0 / S)
    cur = f32(f32(sample) * inc)
    ox, oy = f32(cur + halton(sample, 4)), f32(cur + halton(sample, 5))
    y, x = np.meshgrid(np.arange(row0, row0 + nrows), np.arange(W), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    keys = np_sample_key((x + W * y).astype(U32), U32(sample))
    sampleX = np_rand31(keys, 0).astype(f32) / f32(2147483648.0)
    theta = np_rand31(keys, 1).astype(f32) / f32(2147483647 / (2 * 3.14159265358979323846))
    sn, cs = orc.portable_sincos(theta)
    rad = np.sqrt((sampleX * dof) * dof)
    offx, offy = (rad * cs)[:, None], (rad * sn)[:, None]
    org = (pos[None, :] + up[None, :] * offy) + right[None, :] * offx
    cp = (origin[None, :] + u[None, :] * (x.astype(f32) + ox)[:, None]) + v[None, :] * (y.astype(f32) + oy)[:, None]
    d = cp - org
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    d = d / length[:, None]
    assert all(a.dtype == f32 for a in (org, cp, d, rad, sampleX, theta))
    rays = np.zeros((x.size, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = org, f32(1.0e30), d
    return rays, keys


def test_the_library_exports_the_five_symbols(pkg):
    for name in ("rtu_shade_rays_sampled_device", "rtu_shade_rays_sampled", "rtu_camera_sample_rays", "rtu_sample_key", "rtu_child_key"):
        assert hasattr(pkg.hip, name), "librtu_hip.so does not export " + name
        assert name in pkg.HIP_SYMBOLS


def test_the_key_functions_are_the_headers_formulas(pkg):
    rng = np.random.RandomState(18)
    a = rng.randint(0, 1 << 32, 100000, dtype=np.uint64).astype(U32)
    b = rng.randint(0, 1 << 32, 100000, dtype=np.uint64).astype(U32)
    a[:4] = [0, 1, 0xFFFFFFFF, 0x80000000]
    b[:4] = [0, 0xFFFFFFFF, 0xFFFFFFFF, 1]
    sk, ck = pkg.hip.rtu_sample_key, pkg.hip.rtu_child_key
    got_s = np.array([sk(int(p), int(i)) for p, i in zip(a, b)], U32)
    got_c = np.array([ck(int(p), int(i)) for p, i in zip(a, b)], U32)
    assert np.array_equal(got_s, np_sample_key(a, b))
    assert np.array_equal(got_c, np_child_key(a, b))
    assert pkg.sample_key(7, 3) == int(np_sample_key(7, 3)[0]) and pkg.child_key(7, 2) == int(np_child_key(7, 2)[0])
    # small pixels and samples, the ones a render uses
    p, i = np.meshgrid(np.arange(2000, dtype=U32), np.arange(16, dtype=U32), indexing="ij")
    assert len(np.unique(np_sample_key(p, i))) > 0.999 * p.size  # (a hash: keys of different samples practically never collide)


def frames_under_test(pkg, golden):
    """(name, scene's camera with or without depth of field, W, H)."""
    scene = golden("p10_s4_160x120").scene(pkg)
    flat = clone(pkg, scene)
    flat.desc.camera.dof = 0.0
    lens = clone(pkg, scene)
    lens.desc.camera.dof = 0.35
    lens.desc.camera.focaldist = 21.0
    return [("dof0", flat, 160, 120), ("dof", lens, 160, 120), ("odd", lens, 37, 19)]


@pytest.mark.parametrize("S", [1, 4, 9])
def test_camera_sample_rays_bit_for_bit(pkg, orc, golden, S):
    for name, scene, W, H in frames_under_test(pkg, golden):
        frame = pkg.frame_setup(scene.desc.camera, W, H, samples=S)
        assert (frame.dof > 0) == (name != "dof0")
        for sample in sorted({0, min(1, S - 1), S - 1}):
            rays, keys = pkg.camera_sample_rays(frame, sample)
            want_rays, want_keys = numpy_sample_rays(orc, frame, sample, 0, H)
            got = rays.view(np.float32).reshape(-1, 8)
            assert np.array_equal(keys, want_keys), (name, S, sample)
            bad = int((got.view(U32) != want_rays.view(U32)).any(axis=1).sum())
            assert bad == 0, "%s S=%d sample %d: %d of %d rays differ from the restatement" % (name, S, sample, bad, len(got))
            assert np.all(rays["reserved"] == 0) and np.all(rays["tmax"] == np.float32(1.0e30))
            if name == "dof0":
                assert np.all(got[:, 0:3] == np.array(list(frame.cam_pos), np.float32)[None, :])
            else:
                assert len(np.unique(got[:, 0:3], axis=0)) > 0.9 * len(got)  # every ray has its own lens point
            # row ranges are the rows of the whole image
            for row0, nrows in ((0, 1), (H - 1, 1), (5, 7), (H, 0), (3, 0)):
                r, k = pkg.camera_sample_rays(frame, sample, row0, nrows)
                assert r.tobytes() == rays[row0 * W:(row0 + nrows) * W].tobytes() and np.array_equal(k, keys[row0 * W:(row0 + nrows) * W])
        if S > 1:  # another sample: other keys, other offsets
            r0, k0 = pkg.camera_sample_rays(frame, 0)
            r1, k1 = pkg.camera_sample_rays(frame, S - 1)
            assert not np.any(k0 == k1) and not np.array_equal(r0["dir"], r1["dir"])


def test_shards_are_ignored(pkg, golden):
    scene = golden("p10_s4_160x120").scene(pkg)
    whole = pkg.frame_setup(scene.desc.camera, 64, 40, samples=3)
    shard = pkg.frame_setup(scene.desc.camera, 64, 40, samples=3, shard_rank=1, shard_count=3)
    a, b = pkg.camera_sample_rays(whole, 2), pkg.camera_sample_rays(shard, 2)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_camera_sample_rays_refusals(pkg, golden):
    scene = golden("p10_s4_160x120").scene(pkg)
    f = pkg.frame_setup(scene.desc.camera, 16, 12, samples=4)
    rays = np.zeros(16 * 12, pkg.ray_dtype())
    keys = np.zeros(16 * 12, U32)
    call = pkg.hip.rtu_camera_sample_rays

    def go(frame=f, sample=0, row0=0, nrows=12, r=rays.ctypes.data, k=keys.ctypes.data):
        return call(ctypes.byref(frame) if frame is not None else None, sample, row0, nrows, r, k)
    assert go() == pkg.RTU_OK
    assert go(frame=None) == pkg.RTU_ERR_ARG
    for samples in (0, -1):
        g = pkg.frame_setup(scene.desc.camera, 16, 12, samples=samples)
        assert go(frame=g) == pkg.RTU_ERR_ARG
    for w, h in ((0, 12), (16, 0), (-3, 12)):
        g = pkg.frame_setup(scene.desc.camera, 16, 12, samples=4)
        g.width, g.height = w, h
        assert go(frame=g) == pkg.RTU_ERR_ARG
    assert go(sample=4) == pkg.RTU_ERR_ARG and go(sample=-1) == pkg.RTU_ERR_ARG and go(sample=3) == pkg.RTU_OK
    assert go(row0=-1) == pkg.RTU_ERR_ARG and go(row0=13, nrows=0) == pkg.RTU_ERR_ARG and go(row0=6, nrows=7) == pkg.RTU_ERR_ARG
    assert go(nrows=-1) == pkg.RTU_ERR_ARG and go(row0=12, nrows=0) == pkg.RTU_OK
    assert go(r=None) == pkg.RTU_ERR_ARG and go(k=None) == pkg.RTU_ERR_ARG
    assert go(nrows=0, r=None, k=None) == pkg.RTU_OK
    with pytest.raises(pkg.RtuError):
        pkg.camera_sample_rays(f, 4)


def test_a_null_context_is_an_argument_error(pkg):
    rays = np.zeros(4, pkg.ray_dtype())
    keys = np.zeros(4, U32)
    out = np.zeros((4, 4), np.float32)
    d = pkg.shade_desc()
    hip = pkg.hip
    assert hip.rtu_shade_rays_sampled(None, rays.ctypes.data, keys.ctypes.data, 4, ctypes.byref(d), out.ctypes.data, None) == pkg.RTU_ERR_ARG
    assert hip.rtu_shade_rays_sampled_device(None, 16, 16, 4, ctypes.byref(d), 16, None) == pkg.RTU_ERR_ARG
    assert hip.rtu_shade_rays_sampled(None, None, None, 0, ctypes.byref(d), None, None) == pkg.RTU_ERR_ARG
    assert hip.rtu_shade_rays_sampled_device(None, None, None, 0, None, None, None) == pkg.RTU_ERR_ARG
