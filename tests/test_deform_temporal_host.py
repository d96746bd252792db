"""Temporal accumulation on deforming meshes (include/rtu_render.h), no GPU: the table of rtu_scene_motion_deform against a numpy
binary64 composition, and the host accumulators and motion vectors against the numpy restatement of the motion form.

The deform rule is the motion form's with ONE substitution: where a pixel's entry is RTU_MOTION_DEFORM, what is carried through the
entry is (x, n) — its surface record over the previous vertices — in place of the hit's (p, N), and a record that does not fit gives
no lookup. So the restatement here is np_temporal_motion (tests/test_temporal_motion_host.py) on hits whose p / N are replaced by a
float32 numpy interpolation (NaN where the record does not fit: a point that is not finite has no lookup) under the table with
DEFORM cleared, with the P and N planes of the history put back to the real hit: every other word must agree bit for bit.

Inputs: the oracle's first hits of p5low at 96 x 72 and of its wobbled teapot. The oracle reports neither face nor weights, so the
records are built here: the face by float64 brute force over the mesh's 240 faces, the weights by the walk's own binary32
expressions for that face, and every record is VERIFIED by the consistency law — the float32 interp plus the from-node chain
reproduces the oracle's p bit for bit; a pixel that fails is excluded and the excluded share is capped at 2 % of the mesh pixels.
Last, the effect on the oracle's own path-traced samples of a scene whose teapot deforms."""
import ctypes

import numpy as np
import pytest

from test_denoise_host import bits, oracle_guides
from test_light_lists import world_triangles
from test_gpu_surface import dot3, from_node_chain, to_node_chain
from test_mesh_update_host import clone, deformed_scene, tri_records_numpy
from test_temporal_motion_host import nodes, np_chain, np_temporal_motion
from test_temporal_motion_host import np_project

F = np.float32
STATIC, RESET, DEFORM = 1, 2, 4
W, H = 96, 72
TAG = "p5low_200x150"


def np_interp(arr, idx, bc):
    return (arr[idx[:, 0]] * bc[:, 0:1] + arr[idx[:, 1]] * bc[:, 1:2]) + arr[idx[:, 2]] * bc[:, 2:3]


def mesh_np(scene, m):
    h = scene.mesh(m)

    def arr(ptr, n, ct, dt):
        return np.ctypeslib.as_array(ctypes.cast(ptr, ctypes.POINTER(ct)), (n, 3)).astype(dt)
    return (arr(h.v, h.nv, ctypes.c_float, F), arr(h.f, h.nf, ctypes.c_uint32, np.int64), arr(h.vn, h.nvn, ctypes.c_float, F),
            arr(h.fn, h.nf, ctypes.c_uint32, np.int64))


def brute_force_records(pkg, scene, frame, hits):
    """An RtuRaySurface per pixel and the mask of the verified ones. At a mesh hit the face is the float64 brute-force nearest
    triangle of the hit node; the weights are TriObj::IntersectTriangle's own binary32 expressions for that face (tri_hit,
    rtu_intersect.h, on the record tri_records_numpy restates) on the ray carried into the node. THE CONSISTENCY LAW then verifies the
    record: the float32 interp of the face's vertices, carried up the node chain, is the oracle's p bit for bit. A record that fails
    (the float64 nearest triangle is not the reference's winner: a ray within rounding of an edge) is EXCLUDED: mesh = face = -1."""
    rays = pkg.camera_rays(frame)
    surf = np.zeros(rays.size, pkg.surface_dtype())
    surf["mesh"], surf["face"] = -1, -1
    verified = np.zeros(rays.size, bool)
    nd = nodes(scene)
    hit = (hits["flags"] & 1) != 0
    o = rays["org"][0].astype(np.float64)
    for k in np.unique(hits["node"][hit]):
        if nd[int(k)].obj_type != 3:
            continue
        sel = np.flatnonzero(hit & (hits["node"] == k))
        tri = world_triangles(pkg, scene, int(k))
        e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
        tv = o - tri[:, 0]
        qv = np.cross(tv, e1)
        d = rays["dir"][sel].astype(np.float64)
        pv = np.cross(d[:, None, :], e2[None])
        det = (pv * e1[None]).sum(axis=2)
        inv = 1.0 / np.where(np.abs(det) > 1e-300, det, np.inf)
        u = (pv * tv[None]).sum(axis=2) * inv
        w = (d @ qv.T) * inv
        t = (e2 * qv).sum(axis=1)[None] * inv
        ok = (u > -1e-5) & (w > -1e-5) & (u + w < 1 + 1e-5) & (t > 1e-5)
        t = np.where(ok, t, np.inf)
        best = t.argmin(axis=1)
        found = np.isfinite(t[np.arange(len(sel)), best])
        # the weights of that face as the walk computes them
        m = nd[int(k)].mesh_id
        v, f, vn, fn = mesh_np(scene, m)
        rec = tri_records_numpy(f, v, best)
        A, N = rec[:, 0:3], rec[:, 3:6]
        ax, ay, e1x, e1y, e2x, e2y = (rec[:, j] for j in range(6, 12))
        ru = rec.view(np.uint32)
        rcp = (ru[:, 12].astype(np.uint64) | (ru[:, 13].astype(np.uint64) << np.uint64(32))).view(np.float64)
        axis = ru[:, 14]
        with np.errstate(all="ignore"):
            p, dr = to_node_chain(scene, int(k), rays["org"][sel], rays["dir"][sel])
            tt = dot3(A - p, N) / dot3(dr, N)
            q = p + dr * tt[:, None]
            qx, qy = np.where(axis == 0, q[:, 1], q[:, 0]), np.where(axis == 2, q[:, 1], q[:, 2])
            dx, dy = qx - ax, qy - ay
            apc = ((-e1y) * dx + e1x * dy) * F(0.5)
            abp = ((-dy) * e2x + dx * e2y) * F(0.5)
            bc1 = (apc.astype(np.float64) * rcp).astype(F)
            bc2 = (abp.astype(np.float64) * rcp).astype(F)
            bc3 = (1.0 - bc1.astype(np.float64) - bc2.astype(np.float64)).astype(F)
            bc = np.stack([bc3, bc1, bc2], axis=1)
            pw, _ = from_node_chain(scene, int(k), np_interp(v, f[best], bc), np_interp(vn, fn[best], bc))
        good = found & (bits(pw) == bits(hits["p"][sel])).all(axis=1)
        surf["mesh"][sel] = np.where(good, m, -1)
        surf["face"][sel] = np.where(good, best, -1)
        surf["bc"][sel] = np.where(good[:, None], bc, F(0))
        verified[sel] = good
    return surf, verified


def on_meshes(scene, hits):
    nd = nodes(scene)
    types = np.array([nd[i].obj_type for i in range(scene.desc.n_nodes)])
    hit = (hits["flags"] & 1) != 0
    return hit & (types[np.where(hit, hits["node"], 0)] == 3)


EXCLUDED_CAP = 0.02  # of the mesh pixels of a frame


def verified_records(pkg, scene, frame, hits, what):
    """brute_force_records with the cap on the excluded share asserted."""
    surf, verified = brute_force_records(pkg, scene, frame, hits)
    mesh = on_meshes(scene, hits)
    excluded = float((mesh & ~verified).sum()) / max(int(mesh.sum()), 1)
    print("%s: %d mesh pixels, %.2f %% excluded by the consistency law" % (what, mesh.sum(), 100 * excluded))
    assert mesh.sum() > 300 and excluded < EXCLUDED_CAP, "%s: %.2f %% of the records fail the consistency law" % (what, 100 * excluded)
    return surf


@pytest.fixture(scope="module")
def inputs(pkg, orc, golden):
    """The scene before and after a wobble of the teapot (mesh 0, two nodes), two cameras, and per scene the oracle's guides, the
    brute-force records and a noisy sample."""
    prev = golden(TAG).scene(pkg)
    cur = deformed_scene(pkg, prev, 0, ("wobble", 1))
    moved = clone(pkg, cur)
    cam = moved.desc.camera
    cam.pos[0] += 0.6
    cam.pos[2] += 0.3
    rng = np.random.default_rng(5)
    out = {}
    for name, scene in (("prev", prev), ("cur", cur), ("moved", moved)):
        frame = pkg.frame_setup(scene.desc.camera, W, H)
        hits, albedo = oracle_guides(pkg, orc, scene, W, H)
        rgbz = np.concatenate([albedo[:, :3] * rng.uniform(0.2, 1.8, (W * H, 3)).astype(F), hits["t"][:, None]], axis=1).reshape(H, W, 4).astype(F)
        out[name] = (scene, frame, hits, albedo, verified_records(pkg, scene, frame, hits, name), rgbz)
    return out


def restated(pkg, prev_scene, prev_cam, cur_cam, rgbz, hits, albedo, surf, hist_prev, desc, motion, cap):
    """The rule through np_temporal_motion: (image, history [3, H, W, 4], DEFORM pixels, of them without a fitting record)."""
    nd = nodes(prev_scene)
    n = len(motion)
    hit = (hits["flags"] & 1) != 0
    k = hits["node"]
    in_table = hit & (k >= 0) & (k < n)
    flags = np.where(in_table, motion["flags"][np.clip(k, 0, max(n - 1, 0))] if n else 0, 0)
    deform = in_table & ((flags & DEFORM) != 0)
    hits2 = hits.copy()
    bad = np.zeros(len(hits), bool)
    for node in np.unique(k[deform]):
        sel = np.flatnonzero(deform & (k == node))
        m = nd[int(node)].mesh_id
        v, f, vn, fn = mesh_np(prev_scene, m)
        fits = (surf["mesh"][sel] == m) & (surf["face"][sel] >= 0) & (surf["face"][sel] < len(f))
        face = np.where(fits, surf["face"][sel], 0)
        with np.errstate(all="ignore"):
            x, nn = np_interp(v, f[face], surf["bc"][sel]), np_interp(vn, fn[face], surf["bc"][sel])
        hits2["p"][sel] = np.where(fits[:, None], x, F(np.nan))
        hits2["N"][sel] = nn
        bad[sel] = ~fits
    table = motion.copy()
    isdef = (table["flags"] & DEFORM) != 0
    table["flags"] = np.where(isdef, table["flags"] & ~np.uint32(DEFORM | STATIC), table["flags"])
    out, hist, _ = np_temporal_motion(prev_cam, cur_cam, rgbz, hits2, albedo, hist_prev, desc, table, cap)
    valid = hit.reshape(H, W)
    hist[1][..., :3] = np.where(valid[..., None], hits["p"].reshape(H, W, 3), F(0))
    hist[2][..., :3] = np.where(valid[..., None], hits["N"].reshape(H, W, 3), F(0))
    return out, hist, deform, bad


# ---- 1. the table -----------------------------------------------------------------------------------------------------------------------------
def test_table(pkg, golden, tmp_path):
    from test_gpu_scene_update import torus_scene
    scene = torus_scene(pkg, tmp_path)  # node 1 a group, node 2 its child (the mesh), node 3 the other instance, node 4 the floor
    nd = nodes(scene)
    assert nd[2].parent == 1 and nd[2].mesh_id == nd[3].mesh_id >= 0
    mesh = nd[2].mesh_id
    prev = clone(pkg, scene)
    prev.node_rotate(1, (0.6, 0.0, 0.8), 33.0)
    prev.node_scale(1, 1.4, 0.7, 1.1)  # the parent rotated and scaled non-uniformly
    prev.node_translate(2, (0.2, -0.1, 0.3))
    cur = deformed_scene(pkg, prev, mesh, ("wobble", 1))
    cur.node_translate(1, (0.5, 0.0, 0.0))
    n = cur.desc.n_nodes
    # an empty deform list: rtu_scene_motion's bytes
    for reset in ((), (mesh,)):
        assert pkg.scene_motion(prev, cur, reset, deform_meshes=()).tobytes() == pkg.scene_motion(prev, cur, reset).tobytes()
    t = pkg.scene_motion(prev, cur, deform_meshes=[mesh])
    plain = pkg.scene_motion(prev, cur, reset_meshes=[mesh])
    assert not t["reserved"].any()
    for i in range(n):
        if nd[i].mesh_id != mesh:
            assert t[i].tobytes() == plain[i].tobytes(), "node %d is not of the deforming mesh" % i
            continue
        assert t["flags"][i] == DEFORM
        (Ap, bp), (Api, _) = np_chain(prev, i)
        m = np.concatenate([Ap, bp[:, None]], axis=1)
        for what, got, want in (("m", t["m"][i], m), ("g", t["g"][i], Api.T)):
            # binary64, rounded once: half an ulp; another association of the binary64 products can flip that rounding (one ulp of the
            # row's largest magnitude, the bar of tests/test_temporal_motion_host.py)
            tol = 2.0 ** -23 * np.abs(want).max(axis=1, keepdims=True)
            assert (np.abs(got.astype(np.float64) - want) <= tol).all(), "node %d %s:\n%s\n%s" % (i, what, got, want)
    assert abs(np.linalg.det(t["m"][2][:, :3].astype(np.float64)) - 1.4 * 0.7 * 1.1 * np.linalg.det(np.array(list(nd[2].tm)).reshape(3, 3))) < 1e-3
    # a mesh in both lists is RESET, with rtu_scene_motion's entry
    both = pkg.scene_motion(prev, cur, reset_meshes=[mesh], deform_meshes=[mesh])
    assert both.tobytes() == plain.tobytes()
    # the refusals
    out = np.zeros(n, pkg.motion_dtype())
    ids = (ctypes.c_uint32 * 2)(0, cur.desc.n_meshes)
    call = pkg.hip.rtu_scene_motion_deform
    assert call(prev.desc_ptr, cur.desc_ptr, ids, 1, None, 0, out.ctypes.data) == pkg.RTU_OK
    assert call(prev.desc_ptr, cur.desc_ptr, None, 1, None, 0, out.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(prev.desc_ptr, cur.desc_ptr, ids, -1, None, 0, out.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(prev.desc_ptr, cur.desc_ptr, ids, 2, None, 0, out.ctypes.data) == pkg.RTU_ERR_ARG, "mesh id n_meshes is out of range"
    assert call(prev.desc_ptr, cur.desc_ptr, ids, 1, ids, 2, out.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(None, cur.desc_ptr, ids, 1, None, 0, out.ctypes.data) == pkg.RTU_ERR_ARG
    assert call(prev.desc_ptr, cur.desc_ptr, ids, 1, None, 0, None) == pkg.RTU_ERR_ARG
    other = golden("p10_s4_160x120").scene(pkg)
    assert call(prev.desc_ptr, other.desc_ptr, None, 0, None, 0, out.ctypes.data) == pkg.RTU_ERR_SCENE_SHAPE
    # the motion forms still refuse the new flag
    with pytest.raises(pkg.RtuError):
        pkg.motion_vectors(pkg.frame_setup(cur.desc.camera, 4, 4), np.zeros(16, pkg.hit_dtype()), t, 4, 4)


# ---- 2. the accumulators ------------------------------------------------------------------------------------------------------------------------
def first_history(pkg, inputs, name="prev"):
    scene, frame, hits, albedo, surf, rgbz = inputs[name]
    table = pkg.scene_motion(scene, scene)
    return pkg.temporal_accumulate_motion(None, frame, rgbz, hits, albedo, table, None, pkg.temporal_desc())[1]


@pytest.mark.parametrize("name,cap", [("cur", 0), ("moved", 0), ("moved", 2)])
def test_host_forms_equal_the_restatement(pkg, inputs, name, cap):
    prev_scene, prev_frame = inputs["prev"][:2]
    scene, frame, hits, albedo, surf, rgbz = inputs[name]
    desc = pkg.temporal_desc(sigma_plane=0.1, normal_min=0.8)
    hist0 = first_history(pkg, inputs)
    table = pkg.scene_motion(prev_scene, scene, deform_meshes=[0])
    assert (table["flags"] == DEFORM).sum() == 2
    got = pkg.temporal_accumulate_deform(prev_frame, frame, rgbz, hits, albedo, surf, prev_scene, table, hist0, desc, cap)
    want_img, want_hist, deform, bad = restated(pkg, prev_scene, prev_frame, frame, rgbz, hits, albedo, surf, hist0, desc, table, cap)
    for what, g, w in (("image", got[0], want_img), ("history", got[1], want_hist)):
        diff = bits(g) != bits(w)
        assert not diff.any(), "%s %s: %d words differ, first at %s" % (name, what, diff.sum(), np.argwhere(diff)[0])
    n_hist = got[1][0][..., 3].reshape(-1)
    print("%s cap %d: %d DEFORM pixels, %d without a fitting record, %d of them with history > 1" %
          (name, cap, deform.sum(), bad.sum(), (n_hist[deform] > 1).sum()))
    # (verified records: what finds no history is what a camera move or the wobble uncovers, and silhouettes)
    assert deform.sum() > 300 and (n_hist[deform] > 1).mean() > 0.9, "the deforming teapot keeps its history"
    # the RESET chain on the same inputs restarts those pixels
    reset = pkg.scene_motion(prev_scene, scene, reset_meshes=[0])
    n_reset = pkg.temporal_accumulate_motion(prev_frame, frame, rgbz, hits, albedo, reset, hist0, desc, cap)[1][0][..., 3].reshape(-1)
    assert (n_reset[deform] == 1).all()
    # the moments form: E, P, N and the image are the three-plane form's; M is the moments form's on the substituted point, which
    # the restatement's planes cannot tell apart from the deform form's own (same n_prev, same taps)
    hist0m = np.concatenate([hist0, np.zeros((1, H, W, 4), F)])
    gm = pkg.temporal_accumulate_deform(prev_frame, frame, rgbz, hits, albedo, surf, prev_scene, table, hist0m, desc, cap, moments=True)
    assert np.array_equal(bits(gm[0]), bits(got[0])) and np.array_equal(bits(gm[1][:3]), bits(got[1]))
    assert gm[1][3][..., :2].any() and not gm[1][3][..., 2:].any()


def test_without_deform_entries_it_is_the_motion_form(pkg, inputs):
    prev_scene, prev_frame = inputs["prev"][:2]
    scene, frame, hits, albedo, surf, rgbz = inputs["moved"]
    hist0 = first_history(pkg, inputs)
    desc = pkg.temporal_desc()
    for table in (pkg.scene_motion(prev_scene, scene, reset_meshes=[0]), pkg.scene_motion(prev_scene, prev_scene)):
        want = pkg.temporal_accumulate_motion(prev_frame, frame, rgbz, hits, albedo, table, hist0, desc, 3)
        got = pkg.temporal_accumulate_deform(prev_frame, frame, rgbz, hits, albedo, surf, prev_scene, table, hist0, desc, 3)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        hist0m = np.concatenate([hist0, np.ones((1, H, W, 4), F) * F(0.25)])
        hist0m[3][..., 2:] = 0
        want = pkg.temporal_accumulate_moments(prev_frame, frame, rgbz, hits, albedo, table, hist0m, desc, 3)
        got = pkg.temporal_accumulate_deform(prev_frame, frame, rgbz, hits, albedo, surf, prev_scene, table, hist0m, desc, 3, moments=True)
        assert np.array_equal(bits(got[0]), bits(want[0])) and np.array_equal(bits(got[1]), bits(want[1]))
        mv = pkg.motion_vectors_deform(prev_frame, hits, surf, prev_scene, table, W, H)
        assert np.array_equal(bits(mv), bits(pkg.motion_vectors(prev_frame, hits, table, W, H)))


def test_records_that_do_not_fit_and_a_nan_vertex_give_no_lookup(pkg, inputs):
    prev_scene, prev_frame = inputs["prev"][:2]
    scene, frame, hits, albedo, surf, rgbz = inputs["cur"]
    hist0 = first_history(pkg, inputs)
    desc = pkg.temporal_desc()
    table = pkg.scene_motion(prev_scene, scene, deform_meshes=[0])
    mesh = np.flatnonzero(surf["mesh"] == 0)
    nf = prev_scene.mesh(0).nf
    bad = surf.copy()
    bad["face"][mesh[0::4]] = nf            # one past the last face
    bad["face"][mesh[1::4]] = -7
    bad["face"][mesh[2::4]] = 0x7fffffff
    bad["mesh"][mesh[3::4]] = 1             # another mesh than the node's
    got = pkg.temporal_accumulate_deform(prev_frame, frame, rgbz, hits, albedo, bad, prev_scene, table, hist0, desc)
    want_img, want_hist, deform, nofit = restated(pkg, prev_scene, prev_frame, frame, rgbz, hits, albedo, bad, hist0, desc, table, 0)
    assert nofit.sum() == len(mesh) and np.array_equal(bits(got[0]), bits(want_img)) and np.array_equal(bits(got[1]), bits(want_hist))
    assert (got[1][0][..., 3].reshape(-1)[mesh] == 1).all(), "no lookup: the pixel starts over"
    mv = pkg.motion_vectors_deform(prev_frame, hits, bad, prev_scene, table, W, H).reshape(-1, 4)
    assert not mv[mesh].any()
    # a NaN among the previous vertices: the pixels of its faces have no lookup, nothing faults
    poisoned = clone(pkg, prev_scene)
    v = poisoned.mesh_vertices(0)
    f = mesh_np(prev_scene, 0)[1]
    vertex = int(f[surf["face"][mesh[0]]][0])
    ctypes.cast(poisoned.mesh(0).v, ctypes.POINTER(ctypes.c_float))[3 * vertex] = float("nan")
    got = pkg.temporal_accumulate_deform(prev_frame, frame, rgbz, hits, albedo, surf, poisoned, table, hist0, desc)
    touched = (f[np.clip(surf["face"], 0, nf - 1)] == vertex).any(axis=1) & (surf["mesh"] == 0)
    assert touched.sum() > 0 and (got[1][0][..., 3].reshape(-1)[touched] == 1).all()
    assert np.isfinite(got[0]).all() and v.shape[0] > vertex
    # refusals: a table of another length than the previous scene's node count, NULL records, NULL scene
    with pytest.raises(pkg.RtuError):
        pkg.temporal_accumulate_deform(prev_frame, frame, rgbz, hits, albedo, surf, prev_scene, table[:-1], hist0, desc)
    d = pkg.temporal_desc(W, H)
    out, hist = np.zeros((H, W, 4), F), np.zeros((3, H, W, 4), F)
    call = pkg.hip.rtu_temporal_accumulate_deform
    args = [ctypes.byref(d), ctypes.byref(prev_frame), ctypes.byref(frame), rgbz.ctypes.data, hits.ctypes.data, albedo.ctypes.data, surf.ctypes.data,
            prev_scene.desc_ptr, hist0.ctypes.data, hist.ctypes.data, out.ctypes.data, table.ctypes.data, len(table), 0]
    assert call(*args) == pkg.RTU_OK
    for k in (6, 7, 11):
        broken = list(args)
        broken[k] = None
        assert call(*broken) == pkg.RTU_ERR_ARG


def test_motion_vectors_of_deform_pixels(pkg, inputs):
    prev_scene, prev_frame = inputs["prev"][:2]
    scene, frame, hits, albedo, surf, rgbz = inputs["moved"]
    table = pkg.scene_motion(prev_scene, scene, deform_meshes=[0])
    mv = pkg.motion_vectors_deform(prev_frame, hits, surf, prev_scene, table, W, H)
    nd = nodes(prev_scene)
    deform = (surf["mesh"] == 0)
    want = np.zeros((W * H, 4), F)
    for node in np.unique(hits["node"][deform]):
        sel = np.flatnonzero(deform & (hits["node"] == node))
        v, f, vn, fn = mesh_np(prev_scene, nd[int(node)].mesh_id)
        x = np_interp(v, f[surf["face"][sel]], surf["bc"][sel])
        m = table["m"][node]
        Pm = np.stack([((m[r, 0] * x[:, 0] + m[r, 1] * x[:, 1]) + m[r, 2] * x[:, 2]) + m[r, 3] for r in range(3)], axis=1)
        front, fx, fy = np_project(prev_frame, Pm)
        want[sel] = np.where(front[:, None], np.stack([fx, fy, np.ones_like(fx), np.zeros_like(fx)], axis=1), F(0))
    got = mv.reshape(-1, 4)
    assert np.array_equal(bits(got[deform]), bits(want[deform])) and deform.sum() > 300
    # the teapot did move on screen between the two cameras, and where it is seen in both, the vector points at the same node
    px = np.stack([np.arange(W * H) % W, np.arange(W * H) // W], axis=1).astype(F)
    assert np.abs(got[deform, :2] - px[deform]).max() > 1.0


def test_unchanged_vertices_under_a_deform_entry_accept_what_the_static_entry_accepts(pkg, inputs):
    """A DEFORM node whose previous vertices are the current ones and whose chain did not change, on a moved camera: W_prev of
    interp over the same vertices is the hit point again, up to the rounding of m (composed in binary64, rounded once) against the
    level-by-level from_node — so every pixel must find at least the history the STATIC entry finds."""
    cur_scene, cur_frame, hits0, albedo0, surf0, rgbz0 = inputs["cur"]
    scene, frame, hits, albedo, surf, rgbz = inputs["moved"]  # the same scene seen from a moved camera
    desc = pkg.temporal_desc()
    still = pkg.scene_motion(cur_scene, cur_scene)
    hist0 = pkg.temporal_accumulate_motion(None, cur_frame, rgbz0, hits0, albedo0, still, None, desc)[1]
    t_def = pkg.scene_motion(cur_scene, scene, deform_meshes=[0])
    t_sta = pkg.scene_motion(cur_scene, scene)
    assert (t_sta["flags"] == STATIC).all() and (t_def["flags"] == DEFORM).sum() == 2
    n_def = pkg.temporal_accumulate_deform(cur_frame, frame, rgbz, hits, albedo, surf, cur_scene, t_def, hist0, desc)[1][0][..., 3].reshape(-1)
    n_sta = pkg.temporal_accumulate_motion(cur_frame, frame, rgbz, hits, albedo, t_sta, hist0, desc)[1][0][..., 3].reshape(-1)
    mesh = surf["mesh"] == 0
    found_def, found_sta = int((n_def[mesh] > 1).sum()), int((n_sta[mesh] > 1).sum())
    lost = int((mesh & (n_sta > 1) & ~(n_def > 1)).sum())
    print("unchanged vertices, moved camera: %d mesh pixels; history found by the DEFORM entry at %d, by the STATIC entry at %d; "
          "found by STATIC and not by DEFORM: %d; summed history %.2f against %.2f" % (mesh.sum(), found_def, found_sta, lost, n_def[mesh].sum(), n_sta[mesh].sum()))
    assert mesh.sum() > 300 and found_sta > 0.9 * mesh.sum()
    assert found_def >= found_sta, "the DEFORM entry accepts fewer taps than the STATIC entry"
    assert lost == 0 and n_def[mesh].sum() >= n_sta[mesh].sum()
    assert np.array_equal(bits(n_def[~mesh]), bits(n_sta[~mesh]))


# ---- 3. quality, on the oracle alone ----------------------------------------------------------------------------------------------------------
QW, QH, QFRAMES = 160, 120, 8
# RMSE in linear rgb of the last of eight frames against 256 spp of the last scene: p5low at 160 x 120 as a recipe-P frame, one sample
# per frame, the camera at rest, the low teapot (mesh 0, both of its nodes) wobbled a step further in every frame: ("wobble", k).
# Ratios to the raw last sample. The figures first measured are in MEASURED; the bound is 1.1 x the deformed chain's figure (the oracle
# is deterministic: the 10 % only guard later edits).
#                                  the teapot's 2200 pixels    the whole image
#   raw last sample (RMSE)         0.19912                     0.15776
#   deformed chain                 0.3873                      0.3698
#   RESET chain                    1.0000                      0.5402
# Mean history over the teapot 7.58 of 8 against 1.00; the mean of eight independent samples would give 8^-1/2 = 0.354. At most 0.05 %
# of a frame's records are excluded by the consistency law.
MEASURED = {"deform_mesh": 0.3873, "reset_mesh": 1.0000, "deform_all": 0.3698, "reset_all": 0.5402}


def test_quality_on_the_oracle(pkg, orc, golden):
    base = golden(TAG).scene(pkg)
    desc = pkg.temporal_desc(QW, QH)
    frame = pkg.frame_setup(base.desc.camera, QW, QH, samples=16, gather_bounces=4)
    state = {"deform": [None, None], "reset": [None, None]}
    prev = None
    for k in range(QFRAMES):
        s = deformed_scene(pkg, base, 0, ("wobble", k))
        sample = orc.sample_images(s, QW, QH, 16, k, 1, gi=True, threads=8)[0]
        hits, albedo = oracle_guides(pkg, orc, s, QW, QH)
        surf = verified_records(pkg, s, frame, hits, "frame %d" % k)
        tables = {"deform": pkg.scene_motion(prev if k else s, s, deform_meshes=[0] if k else []),
                  "reset": pkg.scene_motion(prev if k else s, s, reset_meshes=[0] if k else [])}
        for chain, st in state.items():
            st[0], st[1] = pkg.temporal_accumulate_deform(frame if k else None, frame, sample, hits, albedo, surf, prev if k else s, tables[chain], st[1], desc)
        prev = s
    mesh = on_meshes(s, hits).reshape(QH, QW)
    n_def, n_res = state["deform"][1][0][..., 3], state["reset"][1][0][..., 3]
    print("%d teapot pixels: mean history %.2f on the deformed chain, %.2f on the RESET chain" % (mesh.sum(), n_def[mesh].mean(), n_res[mesh].mean()))
    assert mesh.sum() > 1000 and (n_res[mesh] == 1).all()
    ref = orc.render_paths(s, QW, QH, 256, threads=8)[0]

    def rmse(img, mask):
        d2 = (img[..., :3].astype(np.float64) - ref[..., :3].astype(np.float64)) ** 2
        return float(np.sqrt(np.mean(d2[mask])))
    masks = {"mesh": mesh, "all": np.ones((QH, QW), bool)}
    raw = {w: rmse(sample, m) for w, m in masks.items()}
    print("RMSE of the raw last sample: mesh %.5f, all %.5f" % (raw["mesh"], raw["all"]))
    ratios = {"%s_%s" % (chain, w): rmse(st[0], m) / raw[w] for chain, st in state.items() for w, m in masks.items()}
    for key in sorted(ratios):
        print("ratio %s: %.4f" % (key, ratios[key]))
    assert ratios["deform_mesh"] < ratios["reset_mesh"], "the deformed chain is no better than the RESET chain on the mesh"
    assert ratios["deform_mesh"] < 1.1 * MEASURED["deform_mesh"], "deformed chain: ratio %.4f, first measured %.4f" % (ratios["deform_mesh"], MEASURED["deform_mesh"])
