"""The oracle's ray-level entry (rtu_oracle_rays: oracle_binding.trace_rays / occluded_rays / shade_rays) against the oracle's
own renders, and the ray families of tests/test_gpu_rays_oracle.py with the properties that make them worth tracing.

The entry runs Trace / ShadowTrace / Shade — the functions a render calls per pixel, unchanged — on caller-supplied rays. Fed the
pixel-centre rays of a camera it must reproduce that camera's image bit for bit. The families are rays no camera fires: axis-parallel
orthographic grids whose origins lie on the planes of the reference's boxes, probes from inside the scene with exact poles and an
exact equator, tmax within an ulp of the hit, rays that start on surfaces, directions across the accepted unit-length band. What
each family must contain to test anything (non-vacuity) is asserted here, on the oracle alone, before a GPU is involved."""
import ctypes

import numpy as np
import pytest

from test_gpu_ray_query import bits, nodes
from test_mesh_update_host import clone

BIG = np.float32(1.0e30)
CAMERA_TAGS = ["teapot2_240x135", "p4_240x135", "ties_160x120", "mtl_160x120", "p7_200x150", "p13_200x150", "p1_256"]
RTU_OBJ_SPHERE, RTU_OBJ_TRIMESH = 1, 3
IDENTITY = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]


def make_rays(pkg, org, dirs, tmax=BIG):
    org, dirs = np.asarray(org, np.float32), np.asarray(dirs, np.float32)
    n = max(org.reshape(-1, 3).shape[0], dirs.reshape(-1, 3).shape[0])
    rays = np.zeros(n, pkg.ray_dtype())
    rays["org"], rays["dir"], rays["tmax"] = org, dirs, tmax
    return rays


def valid(rays):
    """The rule of include/rtu_render.h restated in binary32 (both sides compile without contraction): finite, tmax > 0,
    |((x x + y y) + z z) - 1| <= 2e-3."""
    d = rays["dir"]
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    assert dd.dtype == np.float32
    fin = np.isfinite(rays["org"]).all(axis=1) & np.isfinite(d).all(axis=1) & np.isfinite(rays["tmax"])
    with np.errstate(invalid="ignore"):
        return fin & (rays["tmax"] > 0) & ~(np.abs(dd - np.float32(1)) > np.float32(2e-3))


def renormalised(d):
    """d / |d| in binary32, twice: |d.d - 1| < 1e-6 afterwards; an exact zero stays an exact zero."""
    d = np.asarray(d, np.float32)
    for _ in range(2):
        d = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
    assert d.dtype == np.float32
    return d


# ---- scenes ----------------------------------------------------------------------------------------------------------------------
def axis_scene(pkg, golden):
    """AXIS: teapot2 with its mesh node (node 1) at the identity — world coordinates are the mesh's object coordinates, an exact
    zero in a world direction is an exact zero in the mesh's object space, and the planes of the mesh's BVH boxes are world planes."""
    scene = clone(pkg, golden("teapot2_240x135").scene(pkg))
    n = nodes(scene)[1]
    assert n.obj_type == RTU_OBJ_TRIMESH and n.parent == 0
    for k in range(9):
        n.tm[k] = n.itm[k] = IDENTITY[k]
    n.pos[0] = n.pos[1] = n.pos[2] = 0.0
    for j in (0, 1):  # the node and its parent: diagonal (the identity, in fact), no translation
        m = nodes(scene)[j]
        assert list(m.tm) == IDENTITY and list(m.itm) == IDENTITY and list(m.pos) == [0.0, 0.0, 0.0]
    return scene


def bvh_planes(scene, mesh=0):
    """Per axis, the distinct plane values of the boxes of RtuMesh.bvh (float32, sorted)."""
    m = scene.mesh(mesh)
    a = np.ctypeslib.as_array(ctypes.cast(m.bvh, ctypes.POINTER(ctypes.c_float)), (m.n_bvh_nodes, 8))[1:]  # node 0 is unused
    return [np.unique(np.concatenate([a[:, k], a[:, 4 + k]])) for k in range(3)]


# ---- family A: orthographic grids with axis-parallel directions ------------------------------------------------------------------
A1_SEED = 1
A1_BATCH = 4096


def family_a1(pkg, scene):
    """Twelve batches of 4096 rays in AXIS: the directions +-e_k, each with the two other components +0.0 and again -0.0. Origins lie
    50 units back along the axis; one free coordinate is a plane value of the mesh's BVH boxes on that axis, the other is uniform
    inside the mesh's bounds for the first half of a batch and a plane value of its own axis for the second half."""
    rng = np.random.RandomState(A1_SEED)
    planes = bvh_planes(scene)
    m = scene.mesh(0)
    lo, hi = list(m.bound_min), list(m.bound_max)
    out = []
    for k in range(3):
        for sign in (1.0, -1.0):
            for zero in (0.0, -0.0):
                a, b = (k + 1) % 3, (k + 2) % 3
                org = np.zeros((A1_BATCH, 3), np.float32)
                org[:, k] = -50.0 * sign
                org[:, a] = rng.choice(planes[a], A1_BATCH)
                org[:, b] = rng.uniform(lo[b], hi[b], A1_BATCH).astype(np.float32)
                org[A1_BATCH // 2:, b] = rng.choice(planes[b], A1_BATCH // 2)
                d = np.full(3, zero, np.float32)
                d[k] = sign
                out.append(("%s%s zeros %+.1f" % ("+" if sign > 0 else "-", "xyz"[k], zero), make_rays(pkg, org, d)))
    return out


def ortho_grid(pkg, centre, d, half, n, back=50.0, outer=()):
    """An n x n orthographic grid of rays along d (used as given: an exactly-zero component stays exactly zero) through the square of
    half-width `half` about `centre`, starting `back` behind it. outer: multiples of `half` at which the outermost grid lines lie
    instead, on both sides — lines that leave a large floor."""
    d = np.asarray(d, np.float64)
    k = int(np.argmin(np.abs(d)))
    u = np.cross(d, np.eye(3)[k])
    u /= np.linalg.norm(u)
    v = np.cross(d, u)
    far = half * np.asarray(outer, np.float64)
    s = np.concatenate([-far[::-1], np.linspace(-half, half, n - 2 * len(far)), far])
    assert len(s) == n
    org = (np.asarray(centre, np.float64) - back * d)[None, None, :] + s[:, None, None] * u[None, None, :] + s[None, :, None] * v[None, None, :]
    return make_rays(pkg, org.reshape(-1, 3), d.astype(np.float32))


A2_DIRS = [(0.0, 0.6, 0.8), (0.6, 0.0, -0.8), (-0.8, 0.6, 0.0), (0.0, -0.6, -0.8), (-0.6, 0.0, 0.8), (0.8, -0.6, 0.0),
           (0.36, 0.48, -0.8)]  # the last: oblique, the control
# centre and half-width of the grids, and the outermost lines (ties: its floor is 60 wide; four lines on each side pass it by)
A2_VIEW = {"AXIS": ((0.0, -2.0, 4.0), 22.0, ()), "ties_160x120": ((0.0, -0.5, 1.0), 7.0, (5.0, 6.0, 7.0, 8.0))}


def family_a2(pkg, name):
    """48 x 48 grids along directions with exactly one zero component (and one oblique control), one batch per direction."""
    centre, half, outer = A2_VIEW[name]
    return [(str(d), ortho_grid(pkg, centre, d, half, 48, back=80.0, outer=outer)) for d in A2_DIRS]


A3_BOX = {"p4_240x135": ((-34.0, -34.0, -22.0), (34.0, 34.0, 46.0)), "teapot2_240x135": ((-14.0, -29.0, -2.0), (16.0, 1.0, 9.0))}


def sphere_faces(scene):
    """Per axis, the exact values centre +- radius (binary32) of every sphere node whose tm is diagonal under ancestors that only
    translate: the planes of that sphere's box in world space."""
    nd, out = nodes(scene), [[], [], []]
    for i in range(scene.desc.n_nodes):
        n = nd[i]
        tm = np.array(list(n.tm), np.float32).reshape(3, 3)
        if n.obj_type != RTU_OBJ_SPHERE or np.count_nonzero(tm - np.diag(np.diag(tm))):
            continue
        c, j, ok = np.array(list(n.pos), np.float32), n.parent, True
        while j >= 0:
            ok = ok and list(nd[j].tm) == IDENTITY
            c = c + np.array(list(nd[j].pos), np.float32)
            j = nd[j].parent
        if not ok:
            continue
        for k in range(3):
            out[k] += [np.float32(c[k] + tm[k, k]), np.float32(c[k] - tm[k, k])]
    return [np.unique(np.array(v, np.float32)) for v in out]


def family_a3(pkg, scene, tag):
    """64 x 64 grids along +-x, +-y, +-z whose grid lines include centre +- radius of every axis-aligned sphere: a ray on such a line
    lies in a face of that sphere's box (0/0 in the box test of the sphere, and of the plane, in object space)."""
    faces = sphere_faces(scene)
    assert all(len(f) >= 2 for f in faces)
    lo, hi = A3_BOX[tag]
    lines = []
    for k in range(3):
        assert len(faces[k]) < 32 and faces[k].min() >= lo[k] and faces[k].max() <= hi[k]
        fill = np.linspace(lo[k], hi[k], 64 - len(faces[k])).astype(np.float32)
        lines.append(np.sort(np.concatenate([faces[k], fill])))
    out = []
    for k in range(3):
        a, b = (k + 1) % 3, (k + 2) % 3
        for sign in (1.0, -1.0):
            org = np.zeros((64, 64, 3), np.float32)
            org[..., k] = (lo[k] - 50.0) if sign > 0 else (hi[k] + 50.0)
            org[..., a] = lines[a][:, None]
            org[..., b] = lines[b][None, :]
            d = np.zeros(3, np.float32)
            d[k] = sign
            out.append(("%s%s" % ("+" if sign > 0 else "-", "xyz"[k]), make_rays(pkg, org.reshape(-1, 3), d)))
    return out


# ---- family B: panoramic probes --------------------------------------------------------------------------------------------------
PROBES = {
    "teapot2_240x135": [(0.0, -10.0, 3.0), (2.5, -8.0, 2.0), (-4.0, -12.0, 2.0), (0.0, -10.0, -3.0)],  # the third: the sphere's centre
    "p4_240x135": [(0.0, 0.0, 12.0), (-5.0, 10.0, 6.5), (7.0, -5.0, 6.5)],                             # the last two: sphere centres
    "mtl_160x120": [(2.0, -3.0, 2.0), (0.0, 0.0, 1.0)],
    "p7_200x150": [(0.0, -10.0, 4.0)],
}
PROBE_OF = {"teapot2_240x135": 0, "p4_240x135": 1, "mtl_160x120": 0, "p7_200x150": 0}  # the probe families C and D start from


def probe_dirs():
    """A latitude-longitude grid of 64 x 33 directions: the poles exactly (0, 0, +-1), the equator row with dir.z == 0 exactly, the
    four meridians through the axes with an exact zero too, renormalised in binary32."""
    theta = np.arange(33)[:, None] * (np.pi / 32.0)
    phi = np.arange(64)[None, :] * (2.0 * np.pi / 64.0)
    d = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta) * np.ones_like(phi)], axis=-1)
    d[np.abs(d) < 1e-12] = 0.0
    d = renormalised(d.reshape(-1, 3).astype(np.float32))
    assert np.all(d[:64] == (0, 0, 1)) and np.all(d[-64:] == (0, 0, -1)) and np.all(d[16 * 64:17 * 64, 2] == 0)
    dd = d.astype(np.float64)
    assert np.abs((dd * dd).sum(axis=1) - 1.0).max() < 1e-6
    return d


def family_b(pkg, tag):
    d = probe_dirs()
    return [(str(o), make_rays(pkg, np.broadcast_to(np.array(o, np.float32), d.shape), d)) for o in PROBES[tag]]


# ---- family C: tmax at the hit ---------------------------------------------------------------------------------------------------
def family_c(pkg, orc, scene, tag):
    """The hit rays of one probe with tmax at, one ulp beyond, one ulp before and at half of the oracle's t; in teapot2 and p4 also
    between the first hit and the second one along the ray (two readings of "midpoint": (t + t2) / 2 with t2 measured from p, and
    t + t2 / 2). Returns [(name, rays)]; the first three are the ones the non-vacuity conditions speak of."""
    probe = family_b(pkg, tag)[PROBE_OF[tag]][1]
    h = orc.trace_rays(scene, probe, threads=4)
    hit = (h["flags"] & orc.RAY_HIT) != 0
    base, t = probe[hit], h["t"][hit]
    assert hit.sum() > 300

    def with_tmax(tm):
        r = base.copy()
        r["tmax"] = tm
        assert valid(r).all()
        return r
    out = [("tmax = t", with_tmax(t)), ("tmax = nextafter(t, +inf)", with_tmax(np.nextafter(t, np.float32(np.inf)))),
           ("tmax = nextafter(t, 0)", with_tmax(np.nextafter(t, np.float32(0)))), ("tmax = t / 2", with_tmax(np.float32(0.5) * t))]
    if tag in ("p4_240x135", "teapot2_240x135"):
        t2 = orc.trace_rays(scene, make_rays(pkg, h["p"][hit], base["dir"]), threads=4)["t"]
        out.append(("tmax = (t + t2) / 2", with_tmax(np.float32(0.5) * (t + t2))))
        out.append(("tmax = t + t2 / 2", with_tmax(t + np.float32(0.5) * t2)))
    return out


# ---- family D: rays that start on surfaces ---------------------------------------------------------------------------------------
def family_d(pkg, orc, scene, tag):
    """From the oracle's p of one probe's hits along N, -N and the mirror direction dir - 2 (dir . N) N (renormalised in binary32).
    Returns (rays, the node each ray starts on)."""
    probe = family_b(pkg, tag)[PROBE_OF[tag]][1]
    h = orc.trace_rays(scene, probe, threads=4)
    hit = (h["flags"] & orc.RAY_HIT) != 0
    p, N, d = h["p"][hit], h["N"][hit], probe["dir"][hit]
    k = np.float32(2) * ((d[:, 0] * N[:, 0] + d[:, 1] * N[:, 1]) + d[:, 2] * N[:, 2])
    rays = np.concatenate([make_rays(pkg, p, N), make_rays(pkg, p, -N), make_rays(pkg, p, renormalised(d - N * k[:, None]))])
    start = np.tile(h["node"][hit], 3)
    ok = valid(rays)  # (a hit with a NaN normal cannot start a valid ray)
    assert ok.sum() > 900
    return rays[ok], start[ok]


# ---- family E: the unit-length band ----------------------------------------------------------------------------------------------
E_N = 6001


def family_e(pkg, tag):
    """6001 random unit directions from a probe origin, scaled by linspace(0.9985, 1.0015): (rays, valid mask by the binary32 rule,
    dot(dir, dir) - 1 in float64)."""
    rng = np.random.RandomState(20261018 + len(tag))
    d = rng.normal(size=(E_N, 3))
    d = renormalised((d / np.linalg.norm(d, axis=1)[:, None]).astype(np.float32))
    d = d * np.linspace(0.9985, 1.0015, E_N).astype(np.float32)[:, None]
    assert d.dtype == np.float32
    rays = make_rays(pkg, np.broadcast_to(np.array(PROBES[tag][0], np.float32), d.shape), d)
    dd = d.astype(np.float64)
    return rays, valid(rays), (dd * dd).sum(axis=1) - 1.0


def scaled_consistency(t, t0, s):
    """A ray whose direction is s times a unit one hits at t0 / s: the largest |t s / t0 - 1| over the rays both of which hit."""
    both = (t != BIG) & (t0 != BIG)
    return float(np.abs(t[both].astype(np.float64) * s[both] / t0[both].astype(np.float64) - 1.0).max()), int(both.sum())


# ==== the entry against the renders ===============================================================================================
def frame_of(pkg, scene, w, h):
    return pkg.frame_setup(scene.desc.camera, w, h)


@pytest.fixture(scope="module")
def cam(pkg, orc, golden):
    """Per tag, once: the scene, its camera rays and eye, the oracle's render of it."""
    cache = {}

    def get(tag):
        if tag not in cache:
            g = golden(tag)
            scene = g.scene(pkg)
            frame = frame_of(pkg, scene, g.width, g.height)
            rays = pkg.camera_rays(frame)
            img, stats = orc.render(scene, g.width, g.height, threads=8)
            img = img.reshape(-1, 4)
            for a in (rays, img):
                a.setflags(write=False)
            cache[tag] = (scene, rays, tuple(frame.cam_pos), img, stats)
        return cache[tag]
    return get


@pytest.mark.parametrize("tag", CAMERA_TAGS)
def test_camera_rays_reproduce_the_render(pkg, orc, cam, tag):
    scene, rays, eye, img, stats = cam(tag)
    assert valid(rays).all()
    out, st = orc.shade_rays(scene, rays, eye, threads=8)
    hit = img[:, 3] != BIG
    assert hit.sum() > 1000
    assert np.array_equal(bits(out[:, 3]), bits(img[:, 3])), "z differs"
    assert np.array_equal(bits(out[hit, :3]), bits(img[hit, :3])), "rgb differs at a hit pixel"
    assert st == stats, "counters differ: %s vs %s" % (st, stats)
    h = orc.trace_rays(scene, rays, threads=8)
    assert np.array_equal(bits(h["t"]), bits(img[:, 3]))
    assert np.array_equal((h["flags"] & orc.RAY_HIT) != 0, hit)
    assert np.array_equal(orc.occluded_rays(scene, rays, threads=8) == 1, hit)
    # the fields of a hit and of a miss
    n_nodes = scene.desc.n_nodes
    mat = np.array([nodes(scene)[i].material_id for i in range(n_nodes)], np.int32)
    assert np.all((h["node"][hit] >= 0) & (h["node"][hit] < n_nodes)) and np.array_equal(h["material"][hit], mat[h["node"][hit]])
    assert np.all(h["flags"][~hit] == 0) and np.all(h["node"][~hit] == -1) and np.all(h["material"][~hit] == -1)
    assert not h["p"][~hit].any() and not h["N"][~hit].any() and not h["pad0"].any() and not h["pad1"].any()
    assert not np.any(h["flags"] & ~np.uint32(orc.RAY_HIT | orc.RAY_FRONT))


def test_a_miss_is_the_environment_map_along_the_ray(pkg, orc, cam):
    scene, rays, eye, img, _ = cam("p7_200x150")
    d = scene.desc
    assert d.environment.has_map and not d.environment.map_is_null and d.environment_map.present
    miss = img[:, 3] == BIG
    assert miss.sum() > 1000
    out = orc.shade_rays(scene, rays, eye, threads=8)[0]
    uvw = orc.texcoords(orc.TEXOP_ENV_UVW, np.ascontiguousarray(rays["dir"][miss]))
    want = np.array(list(d.environment.color), np.float32)[None, :] * orc.texcoords(orc.TEXOP_MAP, uvw, -2, scene)
    assert len(np.unique(want, axis=0)) > 100  # a picture, not a constant
    assert np.array_equal(bits(out[miss, :3]), bits(want.astype(np.float32)))
    assert np.array_equal(bits(out[miss, 3]), bits(rays["tmax"][miss]))
    short = rays[miss].copy()
    short["tmax"] = np.float32(7.5)
    o2 = orc.shade_rays(scene, short, eye)[0]
    assert np.array_equal(bits(o2[:, :3]), bits(out[miss, :3])) and np.all(o2[:, 3] == np.float32(7.5))


def test_a_miss_without_a_map_is_the_environment_colour(pkg, orc, cam):
    scene, rays, eye, img, _ = cam("mtl_160x120")
    d = scene.desc
    assert not d.environment.has_map and list(d.environment.color) != list(d.background.color)
    miss = img[:, 3] == BIG
    assert miss.sum() > 1000
    out = orc.shade_rays(scene, rays, eye, threads=8)[0]
    assert np.all(out[miss, :3] == np.array(list(d.environment.color), np.float32)) and np.all(out[miss, 3] == BIG)
    assert not np.array_equal(bits(out[miss, :3]), bits(img[miss, :3]))  # the render shows the background there


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p4_240x135"])
def test_thread_counts_agree(pkg, orc, cam, tag):
    scene, rays, eye, _, _ = cam(tag)
    rays = rays[::3]  # 10800 rays: no multiple of 8
    want = None
    for threads in (1, 3, 8):
        got = (orc.trace_rays(scene, rays, threads=threads), orc.occluded_rays(scene, rays, threads=threads)) + orc.shade_rays(scene, rays, eye, threads=threads)
        if want is None:
            want = got
            continue
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and got[2].tobytes() == want[2].tobytes()
        assert got[3] == want[3], "counters depend on the thread count"


def test_the_eye_changes_colours_and_no_t(pkg, orc, cam):
    scene, rays, eye, _, _ = cam("p4_240x135")
    rays = rays[::5]
    a = orc.shade_rays(scene, rays, eye, threads=8)[0]
    b = orc.shade_rays(scene, rays, (3.0, -30.0, 9.0), threads=8)[0]
    assert np.array_equal(bits(a[:, 3]), bits(b[:, 3]))
    changed = int((bits(a[:, :3]) != bits(b[:, :3])).any(axis=1).sum())
    print("another eye changes the colour of %d of %d rays" % (changed, len(a)))
    assert changed > 100
    assert list(scene.desc.camera.pos) == list(eye)  # the scene itself is untouched


@pytest.mark.parametrize("k", [0, 2, 5])
def test_max_bounce_through_the_hook(pkg, orc, cam, golden, k):
    scene, rays, eye, _, _ = cam("p4_240x135")
    g = golden("p4_240x135")
    img, stats = orc.render(scene, g.width, g.height, threads=8, max_bounce=k)
    out, st = orc.shade_rays(scene, rays, eye, threads=8, max_bounce=k)
    assert np.array_equal(bits(out), bits(img.reshape(-1, 4)))  # a closed room: every pixel is a hit
    assert st == stats and orc.max_bounce_now() == orc.MAX_BOUNCE


def test_errors(pkg, orc, golden, cam):
    scene, rays, eye, _, _ = cam("p4_240x135")
    assert orc.trace_rays(scene, rays[:0]).size == 0 and orc.shade_rays(scene, rays[:0], eye)[0].shape == (0, 4)
    r = np.ascontiguousarray(rays[:4])
    out = np.zeros((4, 4), np.float32)
    assert orc.lib.rtu_oracle_rays(scene.desc_ptr, r.ctypes.data, 4, None, 3, out.ctypes.data, None, 1) == orc.ERR_ARG
    assert orc.lib.rtu_oracle_rays(scene.desc_ptr, r.ctypes.data, 4, None, orc.RAYS_SHADE, out.ctypes.data, None, 1) == orc.ERR_ARG
    assert orc.lib.rtu_oracle_rays(scene.desc_ptr, None, 4, None, orc.RAYS_CLOSEST, out.ctypes.data, None, 1) == orc.ERR_ARG
    soft = golden("p10_s4_160x120").scene(pkg)  # soft shadows and glossy bounces
    with pytest.raises(orc.OracleError) as e:
        orc.trace_rays(soft, rays[:4])
    assert e.value.code == orc.ERR_STOCHASTIC
    # float32 [n, 8] rows are the same rays
    assert orc.trace_rays(scene, r.view(np.float32).reshape(-1, 8)).tobytes() == orc.trace_rays(scene, r).tobytes()


# ==== non-vacuity of the families =================================================================================================
def hits_of(orc, scene, rays):
    assert valid(rays).all() and rays.size <= 30000
    return (orc.trace_rays(scene, rays, threads=8)["flags"] & orc.RAY_HIT) != 0


def test_family_a1_rays_on_box_planes_change_the_reference_answer(pkg, orc, golden):
    """On rays that lie in planes of the reference's boxes, the reference's box arithmetic hides triangles its triangle test would
    accept: the oracle's t differs from its t with every triangle tested (debug_all_triangles) on at least 50 rays of the family.
    The device's fast walk finds those triangles in its own tree and must still answer as the reference does."""
    scene = axis_scene(pkg, golden)
    fam = family_a1(pkg, scene)
    assert len(fam) == 12
    total = 0
    for name, rays in fam:
        assert rays.size == A1_BATCH and valid(rays).all()
        d = rays["dir"][0]
        assert np.count_nonzero(d) == 1 and np.all(rays["dir"] == d)
        t = orc.trace_rays(scene, rays, threads=8)["t"]
        try:
            orc.debug_all_triangles(True)
            t_all = orc.trace_rays(scene, rays, threads=8)["t"]
        finally:
            orc.debug_all_triangles(False)
        n = int((bits(t) != bits(t_all)).sum())
        hit = t != BIG
        print("A1 %s: %d hits of %d, %d rays whose t the boxes change" % (name, int(hit.sum()), rays.size, n))
        assert hit.sum() > 100 and (~hit).sum() > 100
        total += n
    print("A1: the reference's boxes change t on %d of %d rays" % (total, 12 * A1_BATCH))
    assert total >= 50


@pytest.mark.parametrize("name", ["AXIS", "ties_160x120"])
def test_family_a2_grids_hit_and_miss(pkg, orc, golden, name):
    scene = axis_scene(pkg, golden) if name == "AXIS" else golden(name).scene(pkg)
    for what, rays in family_a2(pkg, name):
        d = rays["dir"][0]
        assert np.count_nonzero(d == 0) == (0 if what == str(A2_DIRS[-1]) else 1) and np.all(rays["dir"] == d)
        hit = hits_of(orc, scene, rays)
        print("A2 %s %s: %d hits of %d" % (name, what, int(hit.sum()), rays.size))
        assert hit.sum() >= 50 and (~hit).sum() >= 50  # (a horizontal grid meets the flat meshes of ties on few lines)


@pytest.mark.parametrize("tag", ["p4_240x135", "teapot2_240x135"])
def test_family_a3_grids_hit_and_miss(pkg, orc, golden, tag):
    scene = golden(tag).scene(pkg)
    faces = sphere_faces(scene)
    print("A3 %s: sphere box faces at x %s, y %s, z %s" % (tag, faces[0], faces[1], faces[2]))
    for what, rays in family_a3(pkg, scene, tag):
        k = "xyz".index(what[1])
        for a in ((k + 1) % 3, (k + 2) % 3):
            assert np.all(np.isin(faces[a], rays["org"][:, a]))  # the exact values are grid lines
        hit = hits_of(orc, scene, rays)
        print("A3 %s %s: %d hits of %d" % (tag, what, int(hit.sum()), rays.size))
        assert hit.sum() > 100 and (~hit).sum() > 100


@pytest.mark.parametrize("tag", sorted(PROBES))
def test_family_b_probes(pkg, orc, golden, tag):
    scene = golden(tag).scene(pkg)
    eye = tuple(scene.desc.camera.pos)
    nan = 0
    for what, rays in family_b(pkg, tag):
        assert rays.size == 64 * 33 and valid(rays).all()
        out = orc.shade_rays(scene, rays, eye, threads=8)[0]
        n = int(np.isnan(out[:, :3]).any(axis=1).sum())
        print("B %s from %s: %d hits of %d, %d NaN colours" % (tag, what, int((out[:, 3] != BIG).sum()), rays.size, n))
        nan += n
    # the reference's own arithmetic gives NaN colours on some of these rays; the device must give them at the same rays
    assert (nan > 0) == (tag in ("mtl_160x120", "p7_200x150"))


def test_family_c_tmax_at_the_hit_goes_both_ways(pkg, orc, golden):
    hits = misses = stale = 0
    for tag in sorted(PROBES):
        scene = golden(tag).scene(pkg)
        for name, rays in family_c(pkg, orc, scene, tag)[:3]:
            h = orc.trace_rays(scene, rays, threads=4)
            hit = (h["flags"] & orc.RAY_HIT) != 0
            at = hit & (bits(h["t"]) == bits(rays["tmax"]))
            print("C %s %s: %d rays, %d hits, %d of them answer t == tmax" % (tag, name, rays.size, int(hit.sum()), int(at.sum())))
            hits, misses, stale = hits + int(hit.sum()), misses + int((~hit).sum()), stale + int(at.sum())
            assert np.all(h["t"][~hit] == rays["tmax"][~hit])
    assert hits > 100 and misses > 100 and stale > 0


@pytest.mark.parametrize("tag", sorted(PROBES))
def test_family_d_rays_from_surfaces(pkg, orc, golden, tag):
    scene = golden(tag).scene(pkg)
    rays, start = family_d(pkg, orc, scene, tag)
    h = orc.trace_rays(scene, rays, threads=4)
    hit = (h["flags"] & orc.RAY_HIT) != 0
    own, near = int((hit & (h["node"] == start)).sum()), int((hit & (h["t"] < np.float32(1e-2))).sum())
    print("D %s: %d rays, %d hits, %d hit the node they start on, %d hits have t < 1e-2" % (tag, rays.size, int(hit.sum()), own, near))
    assert hit.sum() > 100 and (~hit).sum() > 0 and own > 0
    if tag == "teapot2_240x135":
        assert near > 0


@pytest.mark.parametrize("tag", ["p4_240x135", "teapot2_240x135"])
def test_family_e_the_band(pkg, orc, golden, tag):
    scene = golden(tag).scene(pkg)
    rays, ok, excess = family_e(pkg, tag)
    inside_edge = int((ok & (np.abs(np.abs(excess) - 2e-3) < 1e-5)).sum())
    outside_edge = int((~ok & (np.abs(np.abs(excess) - 2e-3) < 1e-5)).sum())
    print("E %s: %d valid, %d invalid, %d / %d within 1e-5 of the boundary inside / outside" % (tag, int(ok.sum()), int((~ok).sum()), inside_edge, outside_edge))
    assert ok.sum() > 500 and (~ok).sum() > 500 and inside_edge >= 20 and outside_edge >= 20
    # 1.0009 and 0.9991 are inside the band, 1.00101 and 0.99899 are not
    for s, want in ((1.0009, True), (0.9991, True), (1.00101, False), (0.99899, False)):
        assert bool(valid(make_rays(pkg, (0, 0, 0), np.array([[0.36, 0.48, -0.8]], np.float32) * np.float32(s)))[0]) == want
    # the oracle answers a scaled ray consistently: t s = t0
    s = np.sqrt(1.0 + excess)
    unit = rays.copy()
    unit["dir"] = renormalised(rays["dir"])
    dev, n = scaled_consistency(orc.trace_rays(scene, rays[ok], threads=4)["t"], orc.trace_rays(scene, unit[ok], threads=4)["t"], s[ok])
    print("E %s: largest |t s / t0 - 1| = %.3g over %d hits" % (tag, dev, n))
    assert n > 500 and dev < 2e-5
