"""rtu_camera_rays, the host-only entry of the ray queries (include/rtu_render.h). No GPU.

The rays must be, bit for bit, what the kernels make of a pixel (primary_pixel: cp = (origin + u * (x + 0.5f)) + v * (y + 0.5f),
dir = normalize(cp - cam_pos), every operation rounded to binary32 in the order of rtu_vec.h). Here that chain is restated with
numpy float32 operations; on the GPU test_gpu_ray_query.py closes the loop (the z of a render equals the t of these rays)."""
import ctypes

import numpy as np
import pytest


def f32(x):
    return np.asarray(x, np.float32)


def expected_rays(frame, row0, nrows):
    """numpy float32 restatement: one IEEE operation per numpy operation, in the order of rtu_vec.h."""
    w = frame.width
    pos, origin, u, v = (f32(list(a)) for a in (frame.cam_pos, frame.origin, frame.u, frame.v))
    x = (np.arange(w, dtype=np.int32).astype(np.float32) + np.float32(0.5))[None, :, None]
    y = (np.arange(row0, row0 + nrows, dtype=np.int32).astype(np.float32) + np.float32(0.5))[:, None, None]
    cp = (origin[None, None, :] + u[None, None, :] * x) + v[None, None, :] * y       # (origin + u * fx) + v * fy
    d = cp - pos[None, None, :]
    dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]      # dot3
    ln = np.sqrt(dd)                                                                  # sqrtf
    d = d / ln[..., None]                                                             # three IEEE divisions
    assert cp.dtype == d.dtype == np.float32
    return d.reshape(-1, 3), pos


def check(pkg, frame, row0, nrows):
    rays = pkg.camera_rays(frame, row0, nrows)
    d, pos = expected_rays(frame, row0, nrows)
    assert rays.shape == (nrows * frame.width,) and rays.dtype.itemsize == 32
    assert np.array_equal(rays["dir"].view(np.uint32), d.view(np.uint32))
    assert np.array_equal(rays["org"].view(np.uint32), np.broadcast_to(pos, d.shape).view(np.uint32))
    assert np.all(rays["tmax"] == np.float32(pkg.RTU_BIGFLOAT)) and np.all(rays["reserved"] == 0)
    # unit length well inside the bound the queries accept
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert np.all(np.abs(dd - np.float32(1)) < 1e-6)
    return rays


def test_camera_rays_full_frame(pkg, golden):
    g = golden("p1_256")
    scene = g.scene(pkg)
    frame = pkg.frame_setup(scene.desc.camera, g.width, g.height)
    rays = check(pkg, frame, 0, g.height)
    assert rays.size == g.width * g.height
    # the default of nrows is "to the bottom"
    assert np.array_equal(pkg.camera_rays(frame).view(np.uint8), rays.view(np.uint8))


def test_camera_rays_odd_frame_and_row_ranges(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    cam = scene.desc.camera
    frame = pkg.frame_setup(cam, 37, 19)
    whole = check(pkg, frame, 0, 19)
    for row0, nrows in ((5, 9), (18, 1), (11, 8), (19, 0)):
        part = check(pkg, frame, row0, nrows)
        assert np.array_equal(part.view(np.uint8), whole[row0 * 37:(row0 + nrows) * 37].view(np.uint8))
    # shards and samples do not enter: the rays are those of the whole image
    sharded = pkg.frame_setup(cam, 37, 19, shard_rank=1, shard_count=2, samples=4)
    assert np.array_equal(pkg.camera_rays(sharded).view(np.uint8), whole.view(np.uint8))


def test_camera_rays_refusals(pkg, golden):
    scene = golden("p1_256").scene(pkg)
    frame = pkg.frame_setup(scene.desc.camera, 16, 8)
    buf = np.zeros(16 * 8, pkg.ray_dtype())
    call = pkg.hip.rtu_camera_rays
    assert call(ctypes.byref(frame), 0, 8, buf.ctypes.data) == pkg.RTU_OK
    assert call(None, 0, 8, buf.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(ctypes.byref(frame), 0, 8, None) == pkg.RTU_ERR_ARG
    assert call(ctypes.byref(frame), 0, 0, None) == pkg.RTU_OK          # nothing to write
    assert call(ctypes.byref(frame), -1, 2, buf.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(ctypes.byref(frame), 0, -1, buf.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(ctypes.byref(frame), 0, 9, buf.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(ctypes.byref(frame), 7, 2, buf.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(ctypes.byref(frame), 9, 0, None) == pkg.RTU_ERR_ARG
    assert call(ctypes.byref(frame), 2 ** 31 - 1, 2 ** 31 - 1, buf.ctypes.data) == pkg.RTU_ERR_ARG   # row0 + nrows must not wrap
    for field in ("width", "height"):
        bad = pkg.RtuFrameDesc.from_buffer_copy(bytes(frame))
        setattr(bad, field, 0)
        assert call(ctypes.byref(bad), 0, 0, None) == pkg.RTU_ERR_ARG
    with pytest.raises(pkg.RtuError):
        pkg.camera_rays(frame, 4, 5)


def test_ray_records_have_the_layout_of_the_header(pkg):
    r, h = pkg.ray_dtype(), pkg.hit_dtype()
    assert r.itemsize == 32 and [r.fields[k][1] for k in ("org", "tmax", "dir", "reserved")] == [0, 12, 16, 28]
    assert h.itemsize == 48 and [h.fields[k][1] for k in ("t", "node", "flags", "material", "p", "N")] == [0, 4, 8, 12, 16, 32]
    assert (pkg.RTU_RAY_HIT, pkg.RTU_RAY_FRONT, pkg.RTU_RAY_INVALID, pkg.RTU_QUERY_REFERENCE_WALK) == (1, 2, 4, 1)
    # float32 [n, 8] rows are accepted as rays; anything else is refused before the library sees it
    a = np.zeros((3, 8), np.float32)
    assert pkg._as_rays(a).shape == (3,)
    with pytest.raises(pkg.RtuError):
        pkg._as_rays(np.zeros((3, 7), np.float32))
    with pytest.raises(pkg.RtuError):
        pkg._as_rays(np.zeros((3, 8), np.float64))
