"""Sensors (include/rtu_render.h, "Sensors"), the part that needs no GPU: the descriptor and its defaults, rtu_sensor_rays of the three
models against a numpy binary32 restatement of the header's expressions — rays and keys bit for bit —, every refusal, and the oracle on
the rays a sensor emits."""
import ctypes

import numpy as np
import pytest

from test_shade_rays_sampled_host import U32, halton, np_sample_key

f32 = np.float32
BIG = f32(1.0e30)
MODELS = ["equirect", "fisheye", "ortho"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def camera_basis(scene):
    """(pos, right, up, forward) of the scene's camera as float32 triples: an orthonormal frame to within binary32 rounding."""
    c = scene.desc.camera
    pos, d, u = (np.array(list(v), np.float64) for v in (c.pos, c.dir, c.up))
    fwd = d / np.linalg.norm(d)
    right = np.cross(fwd, u)
    right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    return tuple(tuple(float(f32(x)) for x in v) for v in (pos, right, up, fwd))


def make(pkg, model, W, H, samples=0, pos=(0.5, -2.0, 1.25), fov_deg=180.0, extent=(3.0, 2.0), **kw):
    """A sensor with a frame that is no axis: right, up, forward = a rotation of x, z, y."""
    a = 0.3
    c, s = float(np.cos(a)), float(np.sin(a))
    return pkg.sensor_desc(model, W, H, pos, (c, s, 0.0), (0.0, 0.0, 1.0), (-s, c, 0.0), samples=samples, fov_deg=fov_deg, extent=extent, **kw)


def offsets(samples, k):
    if samples == 0:
        return f32(0.5), f32(0.5)
    inc = f32(1.0 / samples)
    cur = f32(f32(k) * inc)
    return f32(cur + halton(k, 4)), f32(cur + halton(k, 5))


def norm3(v):
    ln = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    return v / ln[:, None]


def numpy_sensor_rays(orc, d, sample, row0, nrows):
    """The header's expressions in numpy binary32 (every operation on float32 arrays: one rounding each), sincos through the oracle's
    portable_sincos: (rays [n, 8] float32 with reserved 0, keys uint32 [n], outside [n] bool: the fisheye's r > 1)."""
    W, H = d.width, d.height
    v3 = lambda a: np.array(list(a), f32)[None, :]
    pos, right, up, fwd = v3(d.pos), v3(d.right), v3(d.up), v3(d.forward)
    ox, oy = offsets(d.samples, sample)
    y, x = np.meshgrid(np.arange(row0, row0 + nrows), np.arange(W), indexing="ij")
    x, y = x.reshape(-1), y.reshape(-1)
    n = x.size
    keys = np_sample_key((x + W * y).astype(U32), U32(sample))
    xf, yf = x.astype(f32) + ox, y.astype(f32) + oy
    org = np.broadcast_to(pos, (n, 3)).copy()
    outside = np.zeros(n, bool)
    col = lambda a: a[:, None]
    if d.model == 1:
        R = f32(f32(0.5) * f32(min(W, H)))
        dx, dy = (xf - f32(f32(0.5) * f32(W))) / R, (yf - f32(f32(0.5) * f32(H))) / R
        r = np.sqrt(dx * dx + dy * dy)
        outside = r > f32(1)
        a = r * f32(f32(d.fov_deg) * f32(0.008726646))
        sa, ca = orc.portable_sincos(a)
        with np.errstate(all="ignore"):
            direction = norm3(fwd * col(ca) + (right * col(dx / r) + up * col(-(dy / r))) * col(sa))
        direction = np.where(col(r == f32(0)), np.broadcast_to(fwd, (n, 3)), direction)
        direction = np.where(col(outside), f32(0), direction).astype(f32)
    else:
        u, v = xf / f32(W), yf / f32(H)
        if d.model == 0:
            u = np.where(u >= f32(1), u - f32(1), u)
            v = np.where(v > f32(1), f32(1), v)
            sl, cl = orc.portable_sincos(u * f32(6.2831855))
            sp, cp = orc.portable_sincos(v * f32(3.1415927))
            h = fwd * col(-cl) + right * col(-sl)
            direction = norm3(up * col(cp) + h * col(sp))
        else:
            org = (pos + right * col((u - f32(0.5)) * f32(d.extent[0]))) + up * col((f32(0.5) - v) * f32(d.extent[1]))
            direction = np.broadcast_to(fwd, (n, 3)).copy()
    rays = np.zeros((n, 8), f32)
    rays[:, 0:3], rays[:, 3], rays[:, 4:7] = org, BIG, direction
    assert rays.dtype == f32 and org.dtype == f32 and direction.dtype == f32
    return rays, keys, outside


def valid(rays):
    """The ray rule of rtu_render.h on structured rays."""
    d = rays["dir"]
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    fin = np.isfinite(rays["org"]).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(rays["tmax"])
    return fin & (rays["tmax"] > 0) & ~(np.abs(dd - f32(1)) > f32(2e-3))


def test_symbols_and_defaults(pkg):
    for s in ("rtu_sensor_defaults", "rtu_sensor_rays", "rtu_sensor_rays_device", "rtu_render_sensor", "rtu_render_sensor_device"):
        assert s in pkg.HIP_SYMBOLS and hasattr(pkg.hip, s)
    size = ctypes.sizeof(pkg.RtuSensorDesc)
    assert size == 128
    buf = (ctypes.c_uint8 * (size + 64))(*([0xA5] * (size + 64)))
    fn = pkg.hip.rtu_sensor_defaults
    assert ctypes.cast(fn, ctypes.c_void_p).value  # (called through a raw pointer: the signature table wants an RtuSensorDesc)
    raw = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p)(ctypes.cast(fn, ctypes.c_void_p).value)
    assert raw(ctypes.addressof(buf) + 32) == pkg.RTU_OK
    b = bytes(buf)
    assert b[:32] == b"\xA5" * 32 and b[32 + size:] == b"\xA5" * 32, "rtu_sensor_defaults wrote outside the structure"
    d = pkg.RtuSensorDesc.from_buffer_copy(b[32:32 + size])
    assert (d.model, d.width, d.height, d.samples, d.gather_bounces, d.max_bounce, d.flags) == (pkg.RTU_SENSOR_EQUIRECT, 1, 1, 0, 0, 5, 0)
    assert list(d.pos) == [0, 0, 0] and list(d.right) == [1, 0, 0] and list(d.up) == [0, 1, 0] and list(d.forward) == [0, 0, -1]
    assert d.fov_deg == 180.0 and list(d.extent) == [1, 1] and not any(d.reserved)
    assert raw(None) == pkg.RTU_ERR_ARG
    # every byte is written: a second pattern gives the same structure
    buf2 = (ctypes.c_uint8 * size)(*([0x3C] * size))
    assert raw(ctypes.addressof(buf2)) == pkg.RTU_OK and bytes(buf2) == b[32:32 + size]


@pytest.mark.parametrize("model", MODELS)
@pytest.mark.parametrize("size", [(37, 19), (64, 32)])
@pytest.mark.parametrize("samples", [0, 3])
def test_rays_equal_the_restatement(pkg, orc, model, size, samples):
    W, H = size
    d = make(pkg, model, W, H, samples, fov_deg=220.0)
    for k in range(max(samples, 1)):
        rays, keys = pkg.sensor_rays(d, k)
        want, wkeys, outside = numpy_sensor_rays(orc, d, k, 0, H)
        got = np.ascontiguousarray(rays).view(f32).reshape(-1, 8)
        bad = int((bits(got) != bits(want)).any(axis=1).sum())
        assert bad == 0, "%s %dx%d sample %d: %d rays differ from the restatement" % (model, W, H, k, bad)
        assert np.array_equal(keys, wkeys)
        assert np.array_equal(keys, np.array([pkg.sample_key(p, k) for p in range(W * H)], np.uint32))
        assert not rays["reserved"].any() and (rays["tmax"] == BIG).all()
        zero = (rays["dir"] == 0).all(axis=1)
        if model == "fisheye":
            assert np.array_equal(zero, outside)
            assert np.array_equal(valid(rays), ~outside)
            if size == (64, 32):
                assert outside.any() and not outside.all()
        else:
            assert not zero.any() and valid(rays).all()
        # row ranges are slices of the whole
        for row0, nrows in ((0, 1), (5, 7), (H - 1, 1), (H, 0), (3, 0)):
            r2, k2 = pkg.sensor_rays(d, k, row0, nrows)
            assert np.array_equal(r2.view(np.uint8), rays[row0 * W:(row0 + nrows) * W].view(np.uint8))
            assert np.array_equal(k2, keys[row0 * W:(row0 + nrows) * W])


def test_offsets_reach_past_the_last_pixel(pkg, orc):
    """Sample S - 1 of S has offsets above 1 (k / S + Halton): the equirectangular wrap (u >= 1) and clamp (v > 1) are exercised."""
    S = 7
    d = make(pkg, "equirect", 5, 3, S)
    seen_wrap = seen_clamp = False
    for k in range(S):
        ox, oy = offsets(S, k)
        seen_wrap |= bool((f32(4) + ox) / f32(5) >= 1)
        seen_clamp |= bool((f32(2) + oy) / f32(3) > 1)
        rays, _ = pkg.sensor_rays(d, k)
        want, _, _ = numpy_sensor_rays(orc, d, k, 0, 3)
        assert np.array_equal(bits(np.ascontiguousarray(rays).view(f32).reshape(-1, 8)), bits(want))
        assert valid(rays).all()
    assert seen_wrap and seen_clamp


def test_equirect_looks_along_forward_at_the_centre_column(pkg):
    W, H = 37, 19  # odd: the centre column and the centre row are pixel centres (u = v = 0.5 exactly)
    d = make(pkg, "equirect", W, H)
    rays, _ = pkg.sensor_rays(d)
    dirs = rays["dir"].reshape(H, W, 3).astype(np.float64)
    right, up, fwd = (np.array(list(v), np.float64) for v in (d.right, d.up, d.forward))
    assert np.abs(dirs[:, W // 2] @ right).max() < 1e-6 and (dirs[:, W // 2] @ fwd > 0).all()
    assert dirs[H // 2, W // 2] @ fwd > 1 - 1e-6
    assert (dirs[0] @ up > 0.99).all() and (dirs[-1] @ up < -0.99).all()  # the top row looks along up
    assert dirs[H // 2, 0] @ fwd < -0.98  # the seam looks backwards
    assert (rays["org"] == np.array(list(d.pos), f32)).all()


def test_fisheye_centre_and_rim(pkg):
    d = make(pkg, "fisheye", 8, 8, fov_deg=180.0)  # even: no pixel centre at r == 0, the rim at 90 degrees
    rays, _ = pkg.sensor_rays(d)
    fwd = np.array(list(d.forward), np.float64)
    c = rays["dir"].reshape(8, 8, 3).astype(np.float64) @ fwd
    want = np.cos(np.sqrt(2.0) * 0.5 / 4.0 * np.pi / 2.0)  # the four centre pixels: r = sqrt(2) / 8 of the half angle
    assert np.abs(c[3:5, 3:5] - want).max() < 1e-6 and (c[valid(rays).reshape(8, 8)] > -1e-6).all()
    # r == 0 exactly: a 1 x 1 sensor's single pixel centre
    one, _ = pkg.sensor_rays(make(pkg, "fisheye", 1, 1))
    assert np.array_equal(bits(one["dir"][0]), bits(np.array(list(d.forward), f32)))


def test_ortho_window(pkg):
    d = make(pkg, "ortho", 4, 2, extent=(8.0, 2.0))
    rays, _ = pkg.sensor_rays(d)
    pos, right, up = (np.array(list(v), np.float64) for v in (d.pos, d.right, d.up))
    rel = rays["org"].astype(np.float64) - pos
    assert np.allclose(rel @ right, np.tile([-3, -1, 1, 3], 2), atol=1e-5) and np.allclose(rel @ up, np.repeat([0.5, -0.5], 4), atol=1e-5)
    assert (bits(rays["dir"]) == bits(np.array(list(d.forward), f32))).all()


def refusals(pkg):
    """(what, a descriptor that breaks that one rule) for every rule of RtuSensorDesc."""
    def bad(model="equirect", **fields):
        d = make(pkg, model, 8, 4, 2)
        for k, v in fields.items():
            if isinstance(v, tuple):
                getattr(d, k)[:] = v
            else:
                setattr(d, k, v)
        return d
    nan, inf = float("nan"), float("inf")
    out = [("model -1", bad(model=-1)), ("model 3", bad(model=3)), ("width 0", bad(width=0)), ("height 0", bad(height=0)),
           ("height -1", bad(height=-1)), ("2^25 + 1 pixels", bad(width=(1 << 25) + 1, height=1)), ("2^26 pixels", bad(width=1 << 13, height=1 << 13)),
           ("samples -1", bad(samples=-1)), ("samples 65537", bad(samples=65537)), ("gather 1", bad(gather_bounces=1)),
           ("gather 4 without samples", bad(gather_bounces=4, samples=0)), ("max_bounce -1", bad(max_bounce=-1)), ("max_bounce 6", bad(max_bounce=6)),
           ("flag 2", bad(flags=2)), ("reserved[0]", bad(reserved=(1,) + (0,) * 9)), ("reserved[9]", bad(reserved=(0,) * 9 + (1,))),
           ("fov 0", bad("fisheye", fov_deg=0.0)), ("fov 361", bad("fisheye", fov_deg=361.0)), ("fov -90", bad("fisheye", fov_deg=-90.0)),
           ("extent 0", bad("ortho", extent=(0.0, 1.0))), ("extent -1", bad("ortho", extent=(1.0, -1.0)))]
    for field in ("pos", "right", "up", "forward"):
        for v in (nan, inf):
            d = bad()
            getattr(d, field)[1] = v
            out.append(("%s %s" % (field, v), d))
    out += [("fov nan", bad(fov_deg=nan)), ("extent inf", bad(extent=(inf, 1.0)))]  # non-finite is refused whatever the model
    for field in ("right", "up", "forward"):
        d = bad()
        getattr(d, field)[:] = [1.01 * x for x in getattr(d, field)]  # dot = 1.0201
        out.append(("%s too long" % field, d))
    d = bad()
    d.up[:] = (0.0, 0.003, 1.0)  # |up| within the band, up . forward = 0.003 * cos(0.3) > 2e-3
    out.append(("up not orthogonal to forward", d))
    d = bad()
    d.right[:] = list(d.forward)
    out.append(("right == forward", d))
    return out


def test_refusals(pkg):
    rays, keys = np.zeros(64, pkg.ray_dtype()), np.zeros(64, np.uint32)
    call = lambda d, sample=0, row0=0, nrows=1: pkg.hip.rtu_sensor_rays(ctypes.byref(d) if d is not None else None, sample, row0, nrows,
                                                                           rays.ctypes.data, keys.ctypes.data)
    ok = make(pkg, "equirect", 8, 4, 2)
    assert call(ok) == pkg.RTU_OK
    cases = refusals(pkg)
    assert len(cases) == 36
    for what, d in cases:
        assert call(d) == pkg.RTU_ERR_ARG, what
    # within the band: accepted, and used as given
    d = make(pkg, "ortho", 8, 4)
    d.forward[:] = [1.0009 * x for x in d.forward]
    assert call(d) == pkg.RTU_OK and np.array_equal(bits(rays["dir"][0]), bits(np.array(list(d.forward), f32)))
    # fov and extent are read by their own model only
    assert call(make(pkg, "equirect", 8, 4, fov_deg=0.0, extent=(0.0, 0.0))) == pkg.RTU_OK
    assert call(make(pkg, "fisheye", 8, 4, fov_deg=360.0, extent=(0.0, 0.0))) == pkg.RTU_OK
    # the sample, row and pointer rules of rtu_camera_sample_rays
    assert call(None) == pkg.RTU_ERR_ARG
    for kw in (dict(sample=2), dict(sample=-1), dict(row0=-1), dict(row0=5, nrows=0), dict(row0=3, nrows=2), dict(nrows=-1)):
        assert call(ok, **kw) == pkg.RTU_ERR_ARG, kw
    assert call(make(pkg, "equirect", 8, 4, 0), sample=1) == pkg.RTU_ERR_ARG  # samples == 0: sample must be 0
    assert pkg.hip.rtu_sensor_rays(ctypes.byref(ok), 0, 0, 1, None, keys.ctypes.data) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_sensor_rays(ctypes.byref(ok), 0, 0, 1, rays.ctypes.data, None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_sensor_rays(ctypes.byref(ok), 0, 4, 0, None, None) == pkg.RTU_OK
    with pytest.raises(pkg.RtuError):
        pkg.sensor_rays(cases[0][1])
    # a NULL context never reaches a GPU
    assert pkg.hip.rtu_sensor_rays_device(None, ctypes.byref(ok), 0, 1, None, None, None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_render_sensor(None, ctypes.byref(ok), None) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_render_sensor_device(None, ctypes.byref(ok), None, None) == pkg.RTU_ERR_ARG


def scene_sensors(pkg, scene):
    """An equirectangular 64 x 32 sensor at the camera and an orthographic 48 x 48 one across the scene's box, looking as the camera does."""
    pos, right, up, fwd = camera_basis(scene)
    box = pkg.scene_sort_box(scene).astype(np.float64)
    diag = float(np.linalg.norm(box[3:] - box[:3]))
    return (pkg.sensor_desc("equirect", 64, 32, pos, right, up, fwd),
            pkg.sensor_desc("ortho", 48, 48, pos, right, up, fwd, extent=(diag, diag)))


def test_the_oracle_accepts_what_a_sensor_emits(pkg, orc, golden):
    scene = golden("p4_240x135").scene(pkg)
    counts = []
    for d in scene_sensors(pkg, scene):
        rays, _ = pkg.sensor_rays(d)
        assert valid(rays).all()
        out, _ = orc.shade_rays(scene, rays, eye=tuple(d.pos), threads=4)
        assert np.isfinite(out[:, 3]).all() and (out[:, 3] > 0).all()
        hit = out[:, 3] != BIG
        counts.append((int(hit.sum()), int((~hit).sum())))
        assert np.isfinite(out[hit, :3]).all()
    print("p4: (hits, misses) of the equirectangular and the orthographic sensor:", counts)
    assert counts == EXPECTED_P4_COUNTS


EXPECTED_P4_COUNTS = [(92, 1956), (616, 1688)]  # (hits, misses): equirectangular 64 x 32 at the camera, orthographic 48 x 48 across the box
