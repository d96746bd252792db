"""Surface records (rtu_ray_surface / rtu_frame_surface, include/rtu_render.h): which triangle a ray hit and where on it.

  * hits and albedo are the bytes of rtu_ray_features / rtu_frame_features; the reference walk, the fast walk, the fast walk with a
    stack of three entries and the walk without node bounds give the same surface bytes;
  * the record reproduces the hit: the walk's own interpolation restated in float32 numpy from (face, bc), carried up the node chain,
    is RtuRayHit.p and .N bit for bit, and the same weights over vt / ft are uvw — so on an exact tie (ties_160x120) the triangle is
    the one the reference's test order makes the winner;
  * against answers that do not come from the walk: the float64 brute-force nearest triangle (p5low), and the oracle's map sample
    of the reported uvw against the albedo (the textured scenes);
  * spheres, planes, misses and invalid rays; arguments."""
import ctypes

import numpy as np
import pytest

from test_gpu_features import mixed_rays
from test_gpu_ray_query import bits, frame_of, materials, nodes, same_hits
from test_light_lists import world_triangles

pytestmark = pytest.mark.gpu

F = np.float32
TAGS = ["p5low_200x150", "ties_160x120", "mtl_160x120", "p7_200x150"]  # an instanced mesh; exact ties, flat meshes; MultiMtl; textures
RTU_RAY_HIT, RTU_RAY_FRONT, RTU_RAY_INVALID = 1, 2, 4
OBJ_SPHERE, OBJ_PLANE, OBJ_TRIMESH = 1, 2, 3
RTU_MAP_DIFFUSE = 0


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def frames(pkg, golden, ctx):
    """Per scene, computed once: the scene, its frame, and frame_surface / frame_features of it by the default walk."""
    cache = {}

    def get(tag):
        if tag not in cache:
            g = golden(tag)
            scene = g.scene(pkg)
            frame = frame_of(pkg, scene, g.width, g.height)
            ctx.upload(scene)
            cache[tag] = (scene, frame, ctx.frame_surface(frame), ctx.frame_features(frame))
        return cache[tag]
    return get


def raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


# ---- the kernels' float32 expressions (rtu_vec.h, rtu_intersect.h), one rounding per operation, in their order -----------------------
def dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def norm3(a):
    with np.errstate(all="ignore"):
        return a / np.sqrt(dot3(a, a))[:, None]


def mat_mul(m, p):
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    return np.stack([(x * m[0] + y * m[3]) + z * m[6], (x * m[1] + y * m[4]) + z * m[7], (x * m[2] + y * m[5]) + z * m[8]], axis=1)


def mat_tmul(m, d):
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    return np.stack([(m[0] * x + m[1] * y) + m[2] * z, (m[3] * x + m[4] * y) + m[5] * z, (m[6] * x + m[7] * y) + m[8] * z], axis=1)


def interp(arr, idx, bc):
    return (arr[idx[:, 0]] * bc[:, 0:1] + arr[idx[:, 1]] * bc[:, 1:2]) + arr[idx[:, 2]] * bc[:, 2:3]


def node_f32(n):
    return np.array(list(n.tm), F), np.array(list(n.itm), F), np.array(list(n.pos), F)


def chain_up(scene, k):
    """Node k and its ancestors, k first."""
    out, nd = [], nodes(scene)
    while k >= 0:
        out.append(k)
        k = nd[k].parent
    return out


def from_node_chain(scene, k, p, N):
    """Node::FromNodeCoords from node k up to the root (from_node, rtu_intersect.h)."""
    nd = nodes(scene)
    with np.errstate(all="ignore"):
        for j in chain_up(scene, k):
            tm, itm, pos = node_f32(nd[j])
            p = mat_mul(tm, p) + pos
            N = norm3(mat_tmul(itm, N))
    return p, N


def to_node_chain(scene, k, org, d):
    """Node::ToNodeCoords from the root down to node k (to_node)."""
    nd = nodes(scene)
    for j in reversed(chain_up(scene, k)):
        _, itm, pos = node_f32(nd[j])
        p = mat_mul(itm, org - pos)
        d = mat_mul(itm, (org + d) - pos) - p
        org = p
    return org, d


def mesh_arrays(scene, m):
    """v, f, vn, fn, vt, ft of mesh m (vt / ft: None without texture coordinates)."""
    h = scene.mesh(m)

    def arr(ptr, n, ct, dt):
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ct)), (n, 3)).astype(dt) if ptr and n else None
    return (arr(h.v, h.nv, ctypes.c_float, F), arr(h.f, h.nf, ctypes.c_uint32, np.int64), arr(h.vn, h.nvn, ctypes.c_float, F),
            arr(h.fn, h.nf, ctypes.c_uint32, np.int64), arr(h.vt, h.nvt, ctypes.c_float, F),
            arr(h.ft, h.nf, ctypes.c_uint32, np.int64) if h.nvt else None)


def node_types(scene):
    nd = nodes(scene)
    return (np.array([nd[i].obj_type for i in range(scene.desc.n_nodes)]), np.array([nd[i].mesh_id for i in range(scene.desc.n_nodes)]))


def is_miss_record(s):
    return (s["mesh"] == -1) & (s["face"] == -1) & ~bits(s["bc"]).any(axis=1) & ~bits(s["uvw"]).any(axis=1)


# ---- 1. the bytes of the existing entries; every walk the same record -------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_hits_and_albedo_are_the_feature_entries_bytes_and_every_walk_agrees(pkg, orc, ctx, frames, tag):
    import torch
    scene, frame, (hits, albedo, surf), (want_hits, want_albedo) = frames(tag)
    ctx.upload(scene)
    assert same_hits(hits, want_hits) and np.array_equal(raw(albedo), raw(want_albedo))
    rays, valid = mixed_rays(pkg, orc, scene, frame, 5)
    fh, fa = ctx.ray_features(rays)

    def check(what):
        for ref in (False, True):
            h, a, s = ctx.ray_surface(rays, reference_walk=ref)
            assert same_hits(h, fh) and np.array_equal(raw(a), raw(fa)), (what, ref)
            if not (what == "default" and not ref):
                assert np.array_equal(raw(s), raw(check.first)), "%s, reference walk %s: another surface record" % (what, ref)
            else:
                check.first = s
        h, a, s = ctx.frame_surface(frame)
        assert same_hits(h, hits) and np.array_equal(raw(a), raw(albedo)) and np.array_equal(raw(s), raw(surf)), what

    check("default")
    s0 = check.first
    # the camera rays of the batch carry the frame form's records
    cam = pkg.camera_rays(frame)
    assert np.array_equal(raw(ctx.ray_surface(cam)[2]), raw(surf))
    assert is_miss_record(s0[~valid]).all() and (fh["flags"][~valid] == RTU_RAY_INVALID).all()
    back = ((fh["flags"] & RTU_RAY_HIT) != 0) & ((fh["flags"] & RTU_RAY_FRONT) == 0) & (s0["mesh"] >= 0)
    assert back.any(), "no back-face mesh hit in the batch"
    # the device forms: the same bytes, nothing allocated
    n = rays.size
    d_rays = torch.from_numpy(raw(rays).copy()).to("cuda:0")
    d_hits = torch.zeros(max(n, cam.size) * 48, dtype=torch.uint8, device="cuda:0")
    d_alb = torch.full((max(n, cam.size), 4), 7.0, dtype=torch.float32, device="cuda:0")
    d_surf = torch.full((max(n, cam.size) * 32,), 7, dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream(device=0)
    torch.cuda.synchronize()
    a0 = pkg.hip.rtu_debug_device_allocations()
    for ref in (False, True):
        ctx.ray_surface_device(d_rays.data_ptr(), n, d_hits.data_ptr(), d_alb.data_ptr(), d_surf.data_ptr(), stream.cuda_stream, reference_walk=ref)
        stream.synchronize()
        assert np.array_equal(d_hits.cpu().numpy()[:n * 48], raw(fh)) and np.array_equal(raw(d_alb.cpu().numpy()[:n]), raw(fa))
        assert np.array_equal(d_surf.cpu().numpy()[:n * 32], raw(s0))
    ctx.frame_surface_device(frame, d_hits.data_ptr(), d_alb.data_ptr(), d_surf.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    assert np.array_equal(d_hits.cpu().numpy()[:cam.size * 48], raw(hits)) and np.array_equal(d_surf.cpu().numpy()[:cam.size * 32], raw(surf))
    assert pkg.hip.rtu_debug_device_allocations() == a0
    # the fast walk falling back to the reference's tree, and walks without node-level bounds (both hooks last until the next upload)
    assert pkg.hip.rtu_debug_walk_stack_limit(ctx._h, 3) == pkg.RTU_OK
    check("stack limit 3")
    assert pkg.hip.rtu_debug_node_bounds(ctx._h, 0) == pkg.RTU_OK
    check("stack limit 3, no node bounds")
    ctx.upload(scene)
    assert pkg.hip.rtu_debug_node_bounds(ctx._h, 0) == pkg.RTU_OK
    check("no node bounds")
    ctx.upload(scene)


# ---- 2. the record reproduces the hit -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_face_and_weights_reproduce_p_N_and_uvw_bit_for_bit(pkg, frames, tag):
    scene, frame, (hits, albedo, surf), _ = frames(tag)
    types, mesh_of = node_types(scene)
    hit = (hits["flags"] & RTU_RAY_HIT) != 0
    on_mesh = hit & (types[np.where(hit, hits["node"], 0)] == OBJ_TRIMESH)
    assert np.array_equal(on_mesh, surf["mesh"] >= 0), "mesh >= 0 exactly at triangle-mesh hits"
    assert np.array_equal(surf["mesh"][on_mesh], mesh_of[hits["node"][on_mesh]])
    assert on_mesh.sum() > 500
    bc = surf["bc"][on_mesh]
    assert ((bc > 0) & (bc < 1)).all(), "a weight outside (0, 1)"
    err = np.abs(bc.astype(np.float64).sum(axis=1) - 1.0)
    print("%s: %d mesh hits, |bc0 + bc1 + bc2 - 1| <= %.3g" % (tag, on_mesh.sum(), err.max()))
    assert err.max() <= 2 * 2.0 ** -23
    for k in np.unique(hits["node"][on_mesh]):
        sel = np.flatnonzero(on_mesh & (hits["node"] == k))
        v, f, vn, fn, vt, ft = mesh_arrays(scene, int(mesh_of[k]))
        face, w = surf["face"][sel], surf["bc"][sel]
        assert (face >= 0).all() and (face < len(f)).all()
        with np.errstate(all="ignore"):
            p, N = from_node_chain(scene, int(k), interp(v, f[face], w), norm3(interp(vn, fn[face], w)))
        assert np.array_equal(bits(p), bits(hits["p"][sel])), "node %d: p is not the interpolation of the reported face" % k
        assert np.array_equal(bits(N), bits(hits["N"][sel])), "node %d: N is not the interpolation of the reported face" % k
        # (texture coordinates travel to the device with textured scenes only: elsewhere a mesh hit's uvw is 0, as in a render)
        uvw = interp(vt, ft[face], w) if vt is not None and scene.desc.n_textures > 0 else np.zeros((len(sel), 3), F)
        if tag in ("p7_200x150", "mtl_160x120"):
            assert vt is not None and scene.desc.n_textures > 0 and bits(uvw).any()
        assert np.array_equal(bits(uvw), bits(surf["uvw"][sel])), "node %d: uvw" % k
        if tag == "ties_160x120":
            assert len(np.unique(face)) > 20


# ---- 3. against answers that do not come from the walk ------------------------------------------------------------------------------------
def test_the_face_is_the_brute_force_nearest_triangle(pkg, frames):
    scene, frame, (hits, albedo, surf), _ = frames("p5low_200x150")
    types, mesh_of = node_types(scene)
    mesh_nodes = [int(k) for k in np.flatnonzero(types == OBJ_TRIMESH)]
    assert len(mesh_nodes) == 2, "p5low: two nodes of one mesh"
    tri = np.concatenate([world_triangles(pkg, scene, k) for k in mesh_nodes])  # float64 [T, 3, 3]
    nf = len(tri) // 2
    owner = np.repeat(mesh_nodes, nf)
    sel = np.flatnonzero(surf["mesh"] >= 0)
    cam = pkg.camera_rays(frame)
    o = cam["org"][0].astype(np.float64)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    tv = o - tri[:, 0]
    qv = np.cross(tv, e1)
    checked = ambiguous = 0
    for c in range(0, len(sel), 2048):
        idx = sel[c:c + 2048]
        d = cam["dir"][idx].astype(np.float64)
        pv = np.cross(d[:, None, :], e2[None])                      # [n, T, 3]
        det = (pv * e1[None]).sum(axis=2)
        inv = 1.0 / np.where(np.abs(det) > 1e-300, det, np.inf)
        u = (pv * tv[None]).sum(axis=2) * inv
        w = (d @ qv.T) * inv
        t = (e2 * qv).sum(axis=1)[None] * inv
        ok = (np.abs(det) > 1e-300) & (u > -1e-5) & (w > -1e-5) & (u + w < 1 + 1e-5) & (t > 1e-5)
        t = np.where(ok, t, np.inf)
        best = t.argmin(axis=1)
        tmin = t[np.arange(len(idx)), best]
        assert np.isfinite(tmin).all(), "a reported mesh hit that no triangle explains"
        clear = (t < tmin[:, None] + 1e-5).sum(axis=1) == 1
        ambiguous += int((~clear).sum())
        checked += int(clear.sum())
        assert np.array_equal(surf["face"][idx][clear], best[clear] % nf), "another face than the nearest triangle"
        assert np.array_equal(hits["node"][idx][clear], owner[best[clear]])
        assert np.allclose(hits["t"][idx][clear], tmin[clear], rtol=1e-4)
    print("p5low: %d faces checked against the brute force, %d within 1e-5 of a second candidate" % (checked, ambiguous))
    assert checked > 0.8 * len(sel) and checked > 1000


@pytest.mark.parametrize("tag", ["p7_200x150", "mtl_160x120"])
def test_the_oracles_map_sample_of_uvw_is_the_albedo(pkg, orc, frames, tag):
    scene, frame, (hits, albedo, surf), _ = frames(tag)
    d = scene.desc
    assert d.material_maps
    maps = (pkg.RtuTexMap * (4 * d.n_materials)).from_address(d.material_maps)
    front = (hits["flags"] & (RTU_RAY_HIT | RTU_RAY_FRONT)) == (RTU_RAY_HIT | RTU_RAY_FRONT)
    mats, kinds, seen = materials(scene), set(), 0
    types, _ = node_types(scene)
    for m in np.unique(hits["material"][front & (hits["material"] >= 0)]):
        sel = np.flatnonzero(front & (hits["material"] == m))
        colour = np.array(list(mats[int(m)].diffuse), F)
        if maps[4 * int(m) + RTU_MAP_DIFFUSE].present:
            sample = orc.texcoords(pkg.TEXOP_MAP, surf["uvw"][sel], 4 * int(m) + RTU_MAP_DIFFUSE, scene)
            want = (np.zeros(3, F) + (colour * sample) * np.ones(3, F)).astype(F)  # result += diffuse.Sample(uvw) * intensity
            seen += len(sel)
            kinds |= set(types[hits["node"][sel]].tolist())
        else:
            want = np.tile(colour, (len(sel), 1))
        assert np.array_equal(bits(want), bits(albedo[sel, :3])), "material %d: the map at uvw is not the albedo" % m
    print("%s: %d textured front-face hits on object types %s" % (tag, seen, sorted(kinds)))
    assert seen > 500 and OBJ_TRIMESH in kinds


# ---- 4. spheres, planes, misses ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", TAGS)
def test_spheres_planes_and_misses(pkg, ctx, frames, tag):
    scene, frame, (hits, albedo, surf), _ = frames(tag)
    types, _ = node_types(scene)
    hit = (hits["flags"] & RTU_RAY_HIT) != 0
    kind = np.where(hit, types[np.where(hit, hits["node"], 0)], 0)
    assert is_miss_record(surf[~hit]).all(), "a miss is mesh = face = -1 and zeros"
    other = hit & (kind != OBJ_TRIMESH)
    assert (surf["mesh"][other] == -1).all() and (surf["face"][other] == -1).all() and not bits(surf["bc"][other]).any()
    cam = pkg.camera_rays(frame)
    front = (hits["flags"] & RTU_RAY_FRONT) != 0
    n_sphere = n_plane = 0
    for k in np.unique(hits["node"][other]):
        sel = np.flatnonzero(other & (hits["node"] == k))
        p, d = to_node_chain(scene, int(k), cam["org"][sel], cam["dir"][sel])
        q = p + d * hits["t"][sel, None]
        if types[k] == OBJ_SPHERE:  # Sphere::IntersectRay, objFunctions.cpp:38-41: the uv of the node-space normal
            nn = norm3(q)
            N = np.where(front[sel, None], nn, -nn)
            want = ctx.texcoords(pkg.TEXOP_SPHERE_UV, N)
            n_sphere += len(sel)
        else:  # Plane::IntersectRay, :131
            assert types[k] == OBJ_PLANE
            want = np.stack([(q[:, 0] + F(1)) / F(2), (q[:, 1] + F(1)) / F(2), np.zeros(len(sel), F)], axis=1)
            n_plane += len(sel)
        assert np.array_equal(bits(want), bits(surf["uvw"][sel])), "node %d (type %d): uvw" % (k, types[k])
    print("%s: %d sphere, %d plane, %d miss pixels" % (tag, n_sphere, n_plane, (~hit).sum()))
    assert n_plane > 100 and (n_sphere > 100 or tag == "ties_160x120")  # (ties has no sphere)
    assert (~hit).sum() > 1000 or tag == "p5low_200x150"                # (a closed room)


# ---- 5. arguments -----------------------------------------------------------------------------------------------------------------------------
def test_arguments(pkg, golden):
    g = golden("mtl_160x120")
    scene = g.scene(pkg)
    frame = frame_of(pkg, scene, g.width, g.height)
    rays = np.ascontiguousarray(pkg.camera_rays(frame)[:8])
    hits, alb, surf = np.zeros(8, pkg.hit_dtype()), np.zeros((8, 4), F), np.zeros(8, pkg.surface_dtype())
    assert pkg.surface_dtype().itemsize == 32
    n = frame.width * frame.height
    fh, fa, fs = np.zeros(n, pkg.hit_dtype()), np.zeros((n, 4), F), np.zeros(n, pkg.surface_dtype())
    c = pkg.Context(0)
    hip = pkg.hip
    fr = ctypes.byref(frame)
    try:
        assert hip.rtu_ray_surface(c._h, rays.ctypes.data, 8, 0, hits.ctypes.data, alb.ctypes.data, surf.ctypes.data) == pkg.RTU_ERR_NO_SCENE
        assert hip.rtu_ray_surface_device(c._h, 16, 8, 0, 16, 16, 16, None) == pkg.RTU_ERR_NO_SCENE  # (refused before any pointer is read)
        assert hip.rtu_frame_surface(c._h, fr, fh.ctypes.data, fa.ctypes.data, fs.ctypes.data) == pkg.RTU_ERR_NO_SCENE
        assert hip.rtu_frame_surface_device(c._h, fr, 16, 16, 16, None) == pkg.RTU_ERR_NO_SCENE
        c.upload(scene)
        assert hip.rtu_ray_surface(c._h, rays.ctypes.data, 8, 0, hits.ctypes.data, alb.ctypes.data, surf.ctypes.data) == pkg.RTU_OK
        for flags in (2, 4, 0x80000000, 3):
            assert hip.rtu_ray_surface(c._h, rays.ctypes.data, 8, flags, hits.ctypes.data, alb.ctypes.data, surf.ctypes.data) == pkg.RTU_ERR_ARG
            assert hip.rtu_ray_surface_device(c._h, 16, 8, flags, 16, 16, 16, None) == pkg.RTU_ERR_ARG
        for k in range(4):
            args = [rays.ctypes.data, hits.ctypes.data, alb.ctypes.data, surf.ctypes.data]
            args[k] = None
            assert hip.rtu_ray_surface(c._h, args[0], 8, 0, args[1], args[2], args[3]) == pkg.RTU_ERR_ARG
            dev = [16, 16, 16, 16]
            dev[k] = None
            assert hip.rtu_ray_surface_device(c._h, dev[0], 8, 0, dev[1], dev[2], dev[3], None) == pkg.RTU_ERR_ARG
            dev[k] = 24  # not 16-byte aligned
            assert hip.rtu_ray_surface_device(c._h, dev[0], 8, 0, dev[1], dev[2], dev[3], None) == pkg.RTU_ERR_ARG
        assert hip.rtu_ray_surface(c._h, None, 0, 0, None, None, None) == pkg.RTU_OK  # n == 0 launches nothing
        assert hip.rtu_ray_surface_device(c._h, None, 0, 0, None, None, None, None) == pkg.RTU_OK
        assert hip.rtu_ray_surface(None, rays.ctypes.data, 8, 0, hits.ctypes.data, alb.ctypes.data, surf.ctypes.data) == pkg.RTU_ERR_ARG
        assert c.ray_surface(rays[:0])[2].size == 0
        assert hip.rtu_frame_surface(c._h, None, fh.ctypes.data, fa.ctypes.data, fs.ctypes.data) == pkg.RTU_ERR_ARG
        for k in range(3):
            args = [fh.ctypes.data, fa.ctypes.data, fs.ctypes.data]
            args[k] = None
            assert hip.rtu_frame_surface(c._h, fr, args[0], args[1], args[2]) == pkg.RTU_ERR_ARG
            dev = [16, 16, 16]
            dev[k] = None
            assert hip.rtu_frame_surface_device(c._h, fr, dev[0], dev[1], dev[2], None) == pkg.RTU_ERR_ARG
            dev[k] = 8
            assert hip.rtu_frame_surface_device(c._h, fr, dev[0], dev[1], dev[2], None) == pkg.RTU_ERR_ARG
        sharded = pkg.frame_setup(scene.desc.camera, g.width, g.height, shard_rank=1, shard_count=2)
        assert hip.rtu_frame_surface_device(c._h, ctypes.byref(sharded), 16, 16, 16, None) == pkg.RTU_ERR_ARG
        # the host form in chunks of its own buffers: the same records as one batch
        h, a, s = c.frame_surface(frame)
        h2, a2, s2 = c.ray_surface(pkg.camera_rays(frame))
        assert same_hits(h, h2) and np.array_equal(raw(s), raw(s2))
    finally:
        c.close()
