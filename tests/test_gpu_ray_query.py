"""Ray queries (rtu_trace_rays / rtu_occluded_rays, include/rtu_render.h) against the oracle and the renders.

Here the oracle is reached through cameras: a batch of rays is the set of pixel-centre rays of some camera (rtu_camera_rays), and
the oracle's z image of that camera is the expected t, bit for bit. Node identity and occlusion are read off the oracle's colours of
scenes edited so that a colour says which node was hit, or whether a light arrives. Rays no camera fires (axis-parallel grids, probes
from inside the scene, tmax at the hit, rays from surfaces, the unit-length band) are compared field by field with the oracle's
ray-level entry (rtu_oracle_rays) in tests/test_gpu_rays_oracle.py."""
import ctypes

import numpy as np
import pytest

from test_light_lists import RtuLight, RtuNode
from test_mesh_update_host import clone, deformed_scene

pytestmark = pytest.mark.gpu

BIG = np.float32(1.0e30)


class RtuMaterial(ctypes.Structure):
    _fields_ = [("diffuse", ctypes.c_float * 3), ("specular", ctypes.c_float * 3), ("reflection", ctypes.c_float * 3), ("refraction", ctypes.c_float * 3),
                ("emission", ctypes.c_float * 3), ("absorption", ctypes.c_float * 3), ("glossiness", ctypes.c_float), ("ior", ctypes.c_float),
                ("reflection_glossiness", ctypes.c_float), ("refraction_glossiness", ctypes.c_float), ("is_multi_fallback", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


def nodes(scene):
    return ctypes.cast(scene.desc.nodes, ctypes.POINTER(RtuNode))


def lights(scene):
    return ctypes.cast(scene.desc.lights, ctypes.POINTER(RtuLight))


def materials(scene):
    return ctypes.cast(scene.desc.materials, ctypes.POINTER(RtuMaterial))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_hits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def frame_of(pkg, scene, w=None, h=None):
    cam = scene.desc.camera
    return pkg.frame_setup(cam, w or cam.img_width, h or cam.img_height)


def set_camera(scene, pos, target, up=(0.0, 0.0, 1.0), fov=60.0):
    """A look-at camera written into the scene (the oracle renders scene.desc.camera)."""
    p, t, u = (np.asarray(a, np.float64) for a in (pos, target, up))
    d = (t - p) / np.linalg.norm(t - p)
    if abs(np.dot(d, u)) > 0.99:
        u = np.array([0.0, 1.0, 0.0])
    u = u - d * np.dot(u, d)
    u /= np.linalg.norm(u)
    cam = scene.desc.camera
    for k in range(3):
        cam.pos[k], cam.dir[k], cam.up[k] = float(p[k]), float(d[k]), float(u[k])
    cam.fov = fov


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ---- 1. camera rays against the oracle and the render ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["p1_256", "p4_240x135", "teapot2_240x135", "p13_200x150", "ties_160x120"])
def test_camera_rays_give_the_z_of_the_render_and_of_the_oracle(pkg, orc, golden, ctx, tag):
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    frame = frame_of(pkg, scene, g.width, g.height)
    rays = pkg.camera_rays(frame)
    z_gpu = ctx.render(frame)[0][..., 3].reshape(-1)
    z_cpu = orc.render(scene, g.width, g.height, threads=8)[0][..., 3].reshape(-1)
    assert np.array_equal(bits(z_gpu), bits(z_cpu))

    def check(what):
        for ref in (False, True):
            h = ctx.trace_rays(rays, reference_walk=ref)
            bad = int((bits(h["t"]) != bits(z_cpu)).sum())
            print("%s %s ref=%s: t differs from the oracle's z at %d of %d pixels" % (tag, what, ref, bad, z_cpu.size))
            assert bad == 0
            assert np.array_equal(bits(h["t"]), bits(z_gpu))
            assert np.array_equal((h["flags"] & pkg.RTU_RAY_HIT) != 0, z_cpu != BIG)
            assert not np.any(h["flags"] & pkg.RTU_RAY_INVALID)

    check("default")
    if tag in ("ties_160x120", "teapot2_240x135"):
        assert pkg.hip.rtu_debug_walk_stack_limit(ctx._h, 3) == pkg.RTU_OK
        check("stack limit 3")
        assert pkg.hip.rtu_debug_node_bounds(ctx._h, 0) == pkg.RTU_OK
        check("stack limit 3, no node bounds")
        ctx.upload(scene)  # both hooks last until the next upload
        assert pkg.hip.rtu_debug_node_bounds(ctx._h, 0) == pkg.RTU_OK
        check("no node bounds")


# ---- 2. arbitrary origins and directions ----------------------------------------------------------------------------------------
N_CAMERAS, CAM_RES = 24, 16
# where the cameras of a scene are placed: boxes (lo, hi) drawn from in turn. teapot2: around the scene, inside the teapot's box
# (node 1 at (2.5, -8, 0), a teapot some 16 units wide under a uniform scale), below the plane z = 0. p4: inside the room (walls at
# x = +-15, y = 20, z = 0 and 24), in front of it, outside it.
REGIONS = {
    "teapot2_240x135": [((-30, -45, 1), (30, 10, 30)), ((-2, -12, 1), (7, -4, 7)), ((-20, -30, -12), (20, 5, -0.5))],
    "p4_240x135": [((-14, -20, 1), (14, 19, 23)), ((-25, -70, 2), (25, -25, 30)), ((-40, -20, -15), (40, 40, 45))],
}


def random_cameras(tag):
    rng = np.random.RandomState(20260117 + len(tag))
    out = []
    for k in range(N_CAMERAS):
        lo, hi = REGIONS[tag][k % len(REGIONS[tag])]
        pos = rng.uniform(lo, hi)
        target = rng.uniform((-10, -15, 0), (10, 10, 12))
        out.append((pos, target, float(rng.uniform(20, 100))))
    return out


@pytest.fixture(scope="module")
def arbitrary(pkg, orc, golden):
    """Per scene: the scene, the rays of its 24 cameras (16 x 16 each, one batch) and the oracle's z for them. Computed once."""
    out = {}
    for tag in REGIONS:
        scene = golden(tag).scene(pkg)
        rays, zs = [], []
        for pos, target, fov in random_cameras(tag):
            s = clone(pkg, scene)
            set_camera(s, pos, target, fov=fov)
            rays.append(pkg.camera_rays(frame_of(pkg, s, CAM_RES, CAM_RES)))
            zs.append(orc.render(s, CAM_RES, CAM_RES, threads=4)[0][..., 3].reshape(-1))
        rays, zs = np.concatenate(rays), np.concatenate(zs)
        rays.setflags(write=False)
        zs.setflags(write=False)
        out[tag] = (scene, rays, zs)
    return out


@pytest.mark.parametrize("tag", sorted(REGIONS))
def test_arbitrary_rays_against_the_oracle(pkg, ctx, arbitrary, tag):
    scene, rays, z_cpu = arbitrary[tag]
    ctx.upload(scene)
    fast = ctx.trace_rays(rays)
    ref = ctx.trace_rays(rays, reference_walk=True)
    hit = z_cpu != BIG
    print("%s: %d rays, %d hit; t differs from the oracle at %d" % (tag, rays.size, int(hit.sum()), int((bits(fast["t"]) != bits(z_cpu)).sum())))
    assert hit.sum() > 1000 and (~hit).sum() > 0
    assert np.array_equal(bits(fast["t"]), bits(z_cpu))
    assert np.array_equal((fast["flags"] & pkg.RTU_RAY_HIT) != 0, hit)
    assert same_hits(fast, ref), "the fast walk and the reference walk differ in some field"


# ---- 3. hit fields ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(REGIONS))
def test_hit_fields(pkg, ctx, arbitrary, tag):
    """p against org + t * dir in float64: |p - (org + t dir)| <= 1e-4 * max(1, |p|, t), the rounding of the chain of node
    transformations (the largest deviation is printed)."""
    scene, rays, _ = arbitrary[tag]
    ctx.upload(scene)
    h = ctx.trace_rays(rays)
    hit = (h["flags"] & pkg.RTU_RAY_HIT) != 0
    n_nodes = scene.desc.n_nodes
    mat = np.array([nodes(scene)[i].material_id for i in range(n_nodes)], np.int32)
    assert np.all((h["node"][hit] >= 0) & (h["node"][hit] < n_nodes))
    assert np.array_equal(h["material"][hit], mat[h["node"][hit]])
    N = h["N"][hit].astype(np.float64)
    assert np.all(np.abs(np.linalg.norm(N, axis=1) - 1.0) <= 1e-5)
    p = h["p"][hit].astype(np.float64)
    t = h["t"][hit].astype(np.float64)
    q = rays["org"][hit].astype(np.float64) + t[:, None] * rays["dir"][hit].astype(np.float64)
    dev = np.linalg.norm(p - q, axis=1) / np.maximum(1.0, np.maximum(np.linalg.norm(p, axis=1), t))
    print("%s: largest |p - (org + t dir)| / max(1, |p|, t) = %.3g" % (tag, dev.max()))
    assert dev.max() <= 1e-4
    miss = ~hit
    assert np.all(h["flags"][miss] == 0) and np.all(h["node"][miss] == -1) and np.all(h["material"][miss] == -1)
    assert np.all(h["t"][miss] == BIG) and not h["p"][miss].any() and not h["N"][miss].any()
    assert not h["pad0"].any() and not h["pad1"].any()


@pytest.mark.parametrize("tag", ["p4_240x135", "teapot2_240x135", "p13_200x150"])
def test_node_identity_through_the_oracle(pkg, orc, golden, ctx, tag):
    """One ambient light of intensity 1, every material a distinct diffuse colour and nothing else: the oracle's rgb at a hit pixel
    is the diffuse colour of the hit node's material, exactly — hit.material must name it."""
    g = golden(tag)
    scene = g.scene(pkg)
    d = scene.desc
    for m in range(d.n_materials):
        mt = materials(scene)[m]
        ctypes.memset(ctypes.byref(mt), 0, ctypes.sizeof(RtuMaterial))
        mt.diffuse[0], mt.diffuse[1], mt.diffuse[2] = (m + 1) / 16.0, (m + 5) / 32.0, (2 * m + 1) / 64.0
        mt.ior = 1.0
    amb = RtuLight()
    amb.type = 0
    amb.intensity[0] = amb.intensity[1] = amb.intensity[2] = 1.0
    ctypes.memmove(ctypes.byref(lights(scene)[0]), ctypes.byref(amb), ctypes.sizeof(RtuLight))
    d.n_lights = 1
    ctx.upload(scene)
    frame = frame_of(pkg, scene, g.width, g.height)
    h = ctx.trace_rays(pkg.camera_rays(frame))
    rgb = orc.render(scene, g.width, g.height, threads=8)[0][..., :3].reshape(-1, 3)
    hit = (h["flags"] & pkg.RTU_RAY_HIT) != 0
    assert hit.sum() > 1000
    colours = np.array([list(materials(scene)[m].diffuse) for m in range(d.n_materials)] + [[1.0, 1.0, 1.0]], np.float32)  # [-1]: no material
    want = colours[h["material"][hit]]
    # (the light loop of Shade() runs on front faces only: a back face is black)
    front = (h["flags"][hit] & pkg.RTU_RAY_FRONT) != 0
    want = np.where(front[:, None] | (h["material"][hit] < 0)[:, None], want, np.float32(0))
    bad = int((rgb[hit] != want).any(axis=1).sum())
    print("%s: %d hit pixels (%d back faces), %d whose colour is not their material's" % (tag, int(hit.sum()), int((~front).sum()), bad))
    assert bad == 0
    assert len(set(h["material"][hit].tolist())) >= 2


def test_front_flag(pkg, golden, ctx):
    g = golden("p1_256")
    scene = g.scene(pkg)
    ctx.upload(scene)
    # from outside: every hit of these closed objects (spheres) is a front hit
    h = ctx.trace_rays(pkg.camera_rays(frame_of(pkg, scene, 64, 64)))
    hit = (h["flags"] & pkg.RTU_RAY_HIT) != 0
    assert hit.sum() > 100 and np.all(h["flags"][hit] & pkg.RTU_RAY_FRONT)
    # from the centre of sphere node 1: its inside is seen, a back hit
    inside = clone(pkg, scene)
    c = [float(x) for x in nodes(scene)[1].pos]
    set_camera(inside, c, (c[0] + 1.0, c[1] + 0.3, c[2] + 0.2), fov=90.0)
    h = ctx.trace_rays(pkg.camera_rays(frame_of(pkg, inside, 32, 32)))
    own = h["node"] == 1
    assert np.all(h["flags"] & pkg.RTU_RAY_HIT) and own.sum() > 500
    assert not np.any(h["flags"][own] & pkg.RTU_RAY_FRONT)
    rays = pkg.camera_rays(frame_of(pkg, inside, 32, 32))
    assert same_hits(h, ctx.trace_rays(rays, reference_walk=True))
    # ... and with the far side beyond tmax the reference's Sphere::IntersectRay still answers "hit", at its stale z = tmax (the
    # header says so): Trace() and ShadowTrace() of the reference conclude the same for such a ray
    short = rays[own].copy()
    short["tmax"] = h["t"][own] * np.float32(0.5)
    for ref in (False, True):
        hs = ctx.trace_rays(short, reference_walk=ref)
        assert np.all(hs["flags"] & pkg.RTU_RAY_HIT) and np.array_equal(bits(hs["t"]), bits(short["tmax"])) and np.all(hs["node"] == 1)
        assert np.all(ctx.occluded(short, reference_walk=ref) == 1)


# ---- 4. occlusion ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", sorted(REGIONS))
def test_occlusion_is_consistent_with_closest_hit(pkg, ctx, arbitrary, tag):
    scene, rays, _ = arbitrary[tag]
    ctx.upload(scene)
    h = ctx.trace_rays(rays)
    hit = (h["flags"] & pkg.RTU_RAY_HIT) != 0
    for ref in (False, True):
        occ = ctx.occluded(rays, reference_walk=ref)
        assert np.array_equal(occ != 0, hit)
        assert set(np.unique(occ).tolist()) <= {0, 1}
    sel = hit & (h["t"] >= np.float32(1e-2))
    print("%s: %d of %d hits have t >= 1e-2" % (tag, int(sel.sum()), int(hit.sum())))
    assert sel.sum() > 1000
    beyond, short = rays[sel].copy(), rays[sel].copy()
    beyond["tmax"] = h["t"][sel] * np.float32(1.001)
    short["tmax"] = h["t"][sel] * np.float32(0.999)
    for ref in (False, True):
        a, b = ctx.occluded(beyond, reference_walk=ref), ctx.occluded(short, reference_walk=ref)
        print("%s ref=%s: tmax = 1.001 t: %d not occluded; tmax = 0.999 t: %d occluded" % (tag, ref, int((a == 0).sum()), int((b != 0).sum())))
        assert np.all(a == 1)
        assert np.all(b == 0)


def test_occlusion_against_the_oracle(pkg, orc, golden, ctx):
    """teapot2 with white diffuse materials, an ambient light 0.2 and one direct light: the oracle rendered with the direct light at
    intensity 1 and at 0 says, per pixel, whether the light arrives at the primary hit p. The shadow ray of that light is
    {p, BIG, -direction}: the images differ => not occluded; equal and N . (-direction) > 1e-3 => occluded."""
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    d = scene.desc
    for m in range(d.n_materials):
        mt = materials(scene)[m]
        ctypes.memset(ctypes.byref(mt), 0, ctypes.sizeof(RtuMaterial))
        mt.diffuse[0] = mt.diffuse[1] = mt.diffuse[2] = 1.0
        mt.ior = 1.0
    assert d.n_lights == 2 and lights(scene)[1].type == 1
    amb = RtuLight()
    amb.type = 0
    amb.intensity[0] = amb.intensity[1] = amb.intensity[2] = 0.2
    scene.set_light(0, amb)

    def direct(intensity):
        l = RtuLight.from_buffer_copy(bytes(lights(scene)[1]))
        l.intensity[0] = l.intensity[1] = l.intensity[2] = intensity
        scene.set_light(1, l)
    direct(1.0)
    lit = orc.render(scene, g.width, g.height, threads=8)[0][..., :3].reshape(-1, 3)
    direct(0.0)
    unlit = orc.render(scene, g.width, g.height, threads=8)[0][..., :3].reshape(-1, 3)
    differ = (lit != unlit).any(axis=1)
    ctx.upload(scene)
    h = ctx.trace_rays(pkg.camera_rays(frame_of(pkg, scene, g.width, g.height)))
    front = (h["flags"] & (pkg.RTU_RAY_HIT | pkg.RTU_RAY_FRONT)) == (pkg.RTU_RAY_HIT | pkg.RTU_RAY_FRONT)
    L = -np.array(list(lights(scene)[1].vec), np.float32)
    shadow = np.zeros(int(front.sum()), pkg.ray_dtype())
    shadow["org"], shadow["tmax"], shadow["dir"] = h["p"][front], BIG, L
    facing = (h["N"][front].astype(np.float64) @ L.astype(np.float64)) > 1e-3
    must_be_clear, must_be_occluded = differ[front], ~differ[front] & facing
    assert must_be_clear.sum() >= 100 and must_be_occluded.sum() >= 100
    for ref in (False, True):
        occ = ctx.occluded(shadow, reference_walk=ref) != 0
        w1, w2 = int((occ & must_be_clear).sum()), int((~occ & must_be_occluded).sum())
        print("ref=%s: %d lit pixels, %d occluded among them; %d shadowed pixels facing the light, %d not occluded among them" %
              (ref, int(must_be_clear.sum()), w1, int(must_be_occluded.sum()), w2))
        assert w1 == 0 and w2 == 0


# ---- 5. shapes and contract ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teapot(pkg, golden):
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    rays = pkg.camera_rays(frame_of(pkg, scene, g.width, g.height))
    rays.setflags(write=False)
    return scene, rays


def test_batch_sizes(pkg, ctx, teapot):
    scene, rays = teapot
    ctx.upload(scene)
    assert rays.size == 32400
    whole_h, whole_o = ctx.trace_rays(rays), ctx.occluded(rays)
    step = rays.size // 65  # rays from all over the image
    for n in (0, 1, 63, 64, 65, 32400):
        sub = rays[::step][:n] if n < 100 else rays
        want_h, want_o = (whole_h[::step][:n], whole_o[::step][:n]) if n < 100 else (whole_h, whole_o)
        assert sub.size == n
        for ref in (False, True):
            assert same_hits(ctx.trace_rays(sub, reference_walk=ref), want_h), n
            assert np.array_equal(ctx.occluded(sub, reference_walk=ref), want_o), n
    # float32 [n, 8] rows are the same rays
    assert same_hits(ctx.trace_rays(np.ascontiguousarray(rays[:65]).view(np.float32).reshape(-1, 8)), whole_h[:65])
    assert pkg.hip.rtu_trace_rays(ctx._h, None, 0, 0, None) == pkg.RTU_OK
    assert pkg.hip.rtu_occluded_rays_device(ctx._h, None, 0, 0, None, None) == pkg.RTU_OK


def test_invalid_rays_are_flagged_and_not_traced(pkg, ctx, teapot):
    scene, rays = teapot
    ctx.upload(scene)
    good = rays[::97].copy()
    want_h, want_o = ctx.trace_rays(good), ctx.occluded(good)
    bad = good[:14].copy()
    nan, inf = np.float32("nan"), np.float32("inf")
    bad["org"][0, 1] = nan
    bad["dir"][1, 2] = nan
    bad["tmax"][2] = nan
    bad["org"][3, 0] = inf
    bad["dir"][4] = (-inf, 0, 0)
    bad["tmax"][5] = inf
    bad["dir"][6] = 0                       # zero length
    bad["dir"][7] *= np.float32(2)          # length 2
    bad["tmax"][8] = 0
    bad["tmax"][9] = -1
    bad["tmax"][10] = -0.0
    bad["dir"][11] *= np.float32(1.002)     # dot = 1.004: outside the band
    bad["dir"][12] *= np.float32(0.998)
    bad["org"][13] = (-inf, nan, inf)
    n_bad = len(bad)
    # valid rays at the edge of what is accepted: a tiny tmax, a length just inside the band
    edge = good[:3].copy()
    edge["tmax"][0] = np.float32(1e-30)
    edge["dir"][1] *= np.float32(1.0005)
    edge["dir"][2] *= np.float32(0.9995)
    mixed = np.concatenate([good[:40], bad[:7], good[40:], bad[7:], edge])
    is_bad = np.zeros(mixed.size, bool)
    is_bad[40:47] = True
    is_bad[good.size + 7:good.size + n_bad] = True
    is_good = np.zeros(mixed.size, bool)
    is_good[:40] = True
    is_good[47:good.size + 7] = True
    for ref in (False, True):
        h, o = ctx.trace_rays(mixed, reference_walk=ref), ctx.occluded(mixed, reference_walk=ref)
        hb = h[is_bad]
        assert np.all(hb["flags"] == pkg.RTU_RAY_INVALID) and np.all(hb["node"] == -1) and np.all(hb["material"] == -1)
        assert np.array_equal(bits(hb["t"]), bits(mixed["tmax"][is_bad])) and not hb["p"].any() and not hb["N"].any()
        assert not o[is_bad].any()
        assert same_hits(h[is_good], want_h) and np.array_equal(o[is_good], want_o)
        assert not np.any(h[-3:]["flags"] & pkg.RTU_RAY_INVALID)
        assert h[-3]["flags"] == 0 and h[-3]["t"] == np.float32(1e-30)


def test_errors(pkg, teapot):
    scene, rays = teapot
    c = pkg.Context(0)
    try:
        r = np.ascontiguousarray(rays[:8])
        out = np.zeros(8, pkg.hit_dtype())
        occ = np.zeros(8, np.uint8)
        assert pkg.hip.rtu_trace_rays(c._h, r.ctypes.data, 8, 0, out.ctypes.data) == pkg.RTU_ERR_NO_SCENE
        assert pkg.hip.rtu_occluded_rays(c._h, r.ctypes.data, 8, 0, occ.ctypes.data) == pkg.RTU_ERR_NO_SCENE
        assert pkg.hip.rtu_trace_rays_device(c._h, 16, 8, 0, 16, None) == pkg.RTU_ERR_NO_SCENE   # (refused before any pointer is read)
        assert pkg.hip.rtu_occluded_rays_device(c._h, 16, 8, 0, 16, None) == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        assert pkg.hip.rtu_trace_rays(c._h, r.ctypes.data, 8, 0, out.ctypes.data) == pkg.RTU_OK
        for flags in (2, 4, 0x80000000, 3):
            assert pkg.hip.rtu_trace_rays(c._h, r.ctypes.data, 8, flags, out.ctypes.data) == pkg.RTU_ERR_ARG
            assert pkg.hip.rtu_occluded_rays(c._h, r.ctypes.data, 8, flags, occ.ctypes.data) == pkg.RTU_ERR_ARG
            assert pkg.hip.rtu_trace_rays_device(c._h, 16, 8, flags, 16, None) == pkg.RTU_ERR_ARG
            assert pkg.hip.rtu_occluded_rays_device(c._h, 16, 8, flags, 16, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_trace_rays(c._h, None, 8, 0, out.ctypes.data) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_trace_rays(c._h, r.ctypes.data, 8, 0, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_occluded_rays(c._h, r.ctypes.data, 8, 0, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_trace_rays_device(c._h, None, 8, 0, 16, None) == pkg.RTU_ERR_ARG
        assert pkg.hip.rtu_trace_rays_device(c._h, 24, 8, 0, 16, None) == pkg.RTU_ERR_ARG        # not 16-byte aligned
        assert pkg.hip.rtu_trace_rays(None, r.ctypes.data, 8, 0, out.ctypes.data) == pkg.RTU_ERR_ARG
        with pytest.raises(pkg.RtuError):
            c.trace_rays_device(None, 8, None)
    finally:
        c.close()


def test_queries_leave_renders_alone_and_allocate_once(pkg, teapot):
    import torch
    scene, rays = teapot
    c = pkg.Context(0)
    try:
        c.upload(scene)
        frame = frame_of(pkg, scene)
        before = c.render(frame)[0]
        counts = c.frame_counts()
        h1, o1 = c.trace_rays(rays), c.occluded(rays)
        assert c.frame_counts() == counts
        c.frame_status()
        a0 = pkg.hip.rtu_debug_device_allocations()
        h2, o2 = c.trace_rays(rays, reference_walk=True), c.occluded(rays)   # the same size again: the buffers are there
        assert pkg.hip.rtu_debug_device_allocations() == a0
        assert same_hits(h1, h2) and np.array_equal(o1, o2)
        # the device forms, on a stream of the caller's, allocate nothing and equal the host forms
        stream = torch.cuda.Stream(device=0)
        d_rays = torch.from_numpy(np.ascontiguousarray(rays).view(np.uint8).copy()).to("cuda:0")
        d_hits = torch.zeros(rays.size * 48, dtype=torch.uint8, device="cuda:0")
        d_occ = torch.full((rays.size,), 7, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        a0 = pkg.hip.rtu_debug_device_allocations()
        for ref in (False, True):
            c.trace_rays_device(d_rays.data_ptr(), rays.size, d_hits.data_ptr(), stream.cuda_stream, reference_walk=ref)
            c.occluded_device(d_rays.data_ptr(), rays.size, d_occ.data_ptr(), stream.cuda_stream, reference_walk=ref)
            stream.synchronize()
            assert same_hits(d_hits.cpu().numpy().view(pkg.hit_dtype()), h1)
            assert np.array_equal(d_occ.cpu().numpy(), o1)
        assert pkg.hip.rtu_debug_device_allocations() == a0
        assert c.frame_counts() == counts
        after = c.render(frame)[0]
        assert np.array_equal(bits(before), bits(after))
        assert c.frame_counts() == counts
    finally:
        c.close()


def test_queries_follow_scene_updates(pkg, teapot):
    scene, _ = teapot
    c = pkg.Context(0)
    try:
        c.upload(scene)
        frame = frame_of(pkg, scene)
        rays = pkg.camera_rays(frame)
        z0 = c.render(frame)[0][..., 3].reshape(-1)
        moved = clone(pkg, scene)
        moved.node_translate(1, (-3.0, 2.0, 1.5))
        moved.node_rotate(1, (0.2, 0.1, 1.0), 25.0)
        c.update(moved)
        z1 = c.render(frame)[0][..., 3].reshape(-1)
        assert not np.array_equal(bits(z0), bits(z1))
        for ref in (False, True):
            assert np.array_equal(bits(c.trace_rays(rays, reference_walk=ref)["t"]), bits(z1))
        twisted = deformed_scene(pkg, moved, 0, ("twist", 120))
        c.update_meshes(twisted, [0])
        z2 = c.render(frame)[0][..., 3].reshape(-1)
        assert not np.array_equal(bits(z1), bits(z2))
        for ref in (False, True):
            h = c.trace_rays(rays, reference_walk=ref)
            assert np.array_equal(bits(h["t"]), bits(z2))
            assert np.array_equal(c.occluded(rays, reference_walk=ref) != 0, z2 != BIG)
    finally:
        c.close()


def test_two_contexts_answer_alike(pkg, ctx, teapot):
    scene, rays = teapot
    ctx.upload(scene)
    other = pkg.Context(0)
    try:
        other.upload(scene)
        assert same_hits(ctx.trace_rays(rays), other.trace_rays(rays))
        assert np.array_equal(ctx.occluded(rays), other.occluded(rays))
    finally:
        other.close()
