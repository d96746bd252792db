"""The device against the oracle on mirrored, stretched, cancelling and singular node transformations: the families T1-T5 of
tests/test_oracle_transforms.py, which pins the oracle on four of them to the compiled reference and asserts, on the oracle alone,
what each contains. All frames are 96 x 64 or smaller.

Recipe W per scene: the counting variant equals the oracle (z bit for bit, NaN colours at the same pixels, 8-bit RGB within one
level, linear RGB under test_random_scene's 1e-4, counters equal); the fast variant equals the counting variant bit for bit with
stage 2 cooperative and one lane per ray, with and without the node-level bounds (rtu_debug_node_bounds), and with rtu_debug_flags
256 (no tile occupancy), 64 (occluder lists reduced to "empty cell or not") and 4096 (a plane's normal through its chain instead of
from the table of k_plane_normals) — each combination its own figure, printed before the first assertion.
Rays no camera fires (R1-R4 of tests/test_fuzz_host.py) through check_batch of tests/test_gpu_rays_oracle.py; surface records on
the mirrored and the stretched meshes; recipes S and P on stochastic versions of T1 and T2; in-place updates from a benign scene to
T1, T2 and T5 and back; three cameras of T2 in flight."""
import numpy as np
import pytest

from test_fuzz_host import eye_of, ray_families
from test_gpu_far import differing, fast_figures, render_figures, settle
from test_gpu_fuzz import check_paths
from test_gpu_parity import check_against
from test_gpu_ray_query import bits, same_hits
from test_gpu_rays_oracle import check_batch
from test_gpu_scene_update import assert_lists_equal, same_bits
from test_gpu_surface import from_node_chain, interp, mesh_arrays, node_types, norm3
from test_light_lists import world_triangles
from test_mesh_update_host import clone
from test_oracle_rays import frame_of
from test_oracle_transforms import ALL, H, W, load, nodes, scene_of, t5_aspect, transformed, xf_dir  # noqa: F401  (xf_dir: the fixture)

pytestmark = pytest.mark.gpu

FLAGS = (0, 256, 64, 4096)
REL_TOL = 1e-4  # test_random_scene's bar of the linear colours
OBJ_TRIMESH = 3


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


# ---- recipe W ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ALL)
def test_recipe_w(pkg, orc, ctx, xf_dir, label):  # noqa: F811
    scene, _ = scene_of(pkg, xf_dir, label)
    ctx.upload(scene)
    fig, cnt, cpu = render_figures(pkg, orc, ctx, scene, W, H, label, flags=FLAGS)
    settle(orc, [fig], [(cnt, cpu)], rel_tol=REL_TOL)


@pytest.mark.parametrize("label", ["T1", "T2"])
def test_recipe_w_at_a_ragged_size(pkg, orc, ctx, xf_dir, label):  # noqa: F811
    scene, _ = scene_of(pkg, xf_dir, label)
    ctx.upload(scene)
    fig, cnt, cpu = render_figures(pkg, orc, ctx, scene, 61, 45, label + " ragged", flags=FLAGS)
    settle(orc, [fig], [(cnt, cpu)], rel_tol=REL_TOL)


# ---- rays no camera fires ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["T1", "T2", "T4", "T4 compact"])
def test_ray_families(pkg, orc, ctx, xf_dir, label):  # noqa: F811
    """t, node, flags, material, p and N bit for bit, the occlusion byte, the radiance, from the fast walk and the reference walk
    (check_batch); uvw, face and weights through the surface records of both walks; a sorted batch answers with the same bytes.
    The colours keep test_random_scene's bar although R1 and R2 start inside glass (measured: 5.1e-7 at most, NOTEBOOK.md section 23)."""
    scene, _ = scene_of(pkg, xf_dir, label)
    fam = ray_families(pkg, orc, scene, 2)
    eye = eye_of(scene)
    ctx.upload(scene)
    for name, rays in fam:
        hit = check_batch(pkg, orc, ctx, scene, rays, eye, "%s %s" % (label, name), rel_tol=REL_TOL)
        assert hit.any()
        a, b = ctx.ray_surface(rays), ctx.ray_surface(rays, reference_walk=True)
        assert same_hits(a[0], b[0]) and np.array_equal(a[2].view(np.uint8), b[2].view(np.uint8)), "%s %s: the walks' surface records differ" % (label, name)
        assert same_hits(a[0], ctx.trace_rays(rays))
        assert same_hits(ctx.trace_rays(rays, sort=True), a[0]), "sorted closest hits differ"
        assert np.array_equal(ctx.occluded(rays, sort=True), ctx.occluded(rays)), "sorted occlusion bytes differ"
        assert np.array_equal(ctx.shade_rays(rays, eye, sort=True)[0].view(np.uint8), ctx.shade_rays(rays, eye)[0].view(np.uint8)), "sorted radiance differs"


# ---- surface records ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ["T1", "T2"])
def test_surface_records_on_mirrored_and_stretched_meshes(pkg, ctx, xf_dir, label):  # noqa: F811
    """As tests/test_gpu_surface.py on its scenes: (face, weights) reproduce p, N and uvw bit for bit through the node's chain — a
    normal through a mirrored or a thousandfold stretched inverse — and the face is the binary64 brute-force nearest triangle."""
    scene, _ = scene_of(pkg, xf_dir, label)
    ctx.upload(scene)
    frame = frame_of(pkg, scene, W, H)
    hits, _, surf = ctx.frame_surface(frame)
    types, mesh_of = node_types(scene)
    hit = (hits["flags"] & pkg.RTU_RAY_HIT) != 0
    on_mesh = hit & (types[np.where(hit, hits["node"], 0)] == OBJ_TRIMESH)
    assert np.array_equal(on_mesh, surf["mesh"] >= 0) and on_mesh.sum() > 500
    mesh_nodes = [int(k) for k in np.unique(hits["node"][on_mesh])]
    assert len(mesh_nodes) == 3
    for k in mesh_nodes:
        sel = np.flatnonzero(on_mesh & (hits["node"] == k))
        v, f, vn, fn, vt, ft = mesh_arrays(scene, int(mesh_of[k]))
        face, w = surf["face"][sel], surf["bc"][sel]
        with np.errstate(all="ignore"):
            p, N = from_node_chain(scene, k, interp(v, f[face], w), norm3(interp(vn, fn[face], w)))
        assert np.array_equal(bits(p), bits(hits["p"][sel])), "node %d: p is not the interpolation of the reported face" % k
        assert np.array_equal(bits(N), bits(hits["N"][sel])), "node %d: N is not the interpolation of the reported face" % k
        uvw = interp(vt, ft[face], w)
        assert bits(uvw).any() and np.array_equal(bits(uvw), bits(surf["uvw"][sel])), "node %d: uvw" % k
    # the brute force over the world triangles of the three nodes
    tri = np.concatenate([world_triangles(pkg, scene, k) for k in mesh_nodes])
    nf = len(tri) // 3
    owner = np.repeat(mesh_nodes, nf)
    sel = np.flatnonzero(on_mesh)
    cam = pkg.camera_rays(frame)
    o, d = cam["org"][0].astype(np.float64), cam["dir"][sel].astype(np.float64)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    tv = o - tri[:, 0]
    qv = np.cross(tv, e1)
    pv = np.cross(d[:, None, :], e2[None])
    det = (pv * e1[None]).sum(axis=2)
    inv = 1.0 / np.where(np.abs(det) > 1e-300, det, np.inf)
    u, ww, t = (pv * tv[None]).sum(axis=2) * inv, (d @ qv.T) * inv, (e2 * qv).sum(axis=1)[None] * inv
    ok = (np.abs(det) > 1e-300) & (u > -1e-5) & (ww > -1e-5) & (u + ww < 1 + 1e-5) & (t > 1e-5)
    t = np.where(ok, t, np.inf)
    best = t.argmin(axis=1)
    tmin = t[np.arange(len(sel)), best]
    assert np.isfinite(tmin).all(), "a reported mesh hit that no triangle explains"
    clear = (t < tmin[:, None] + 1e-5).sum(axis=1) == 1
    print("%s: %d mesh hits, %d within 1e-5 of a second candidate" % (label, len(sel), int((~clear).sum())))
    assert clear.sum() > 0.8 * len(sel)
    assert np.array_equal(surf["face"][sel][clear], best[clear] % nf), "another face than the nearest triangle"
    assert np.array_equal(hits["node"][sel][clear], owner[best[clear]])
    assert np.allclose(hits["t"][sel][clear], tmin[clear], rtol=1e-4)


# ---- recipes S and P ---------------------------------------------------------------------------------------------------------------
def stochastic(pkg, d, label):
    """The family with the reference's stochastic attributes: glossy mirrors (the card, the ball in the mirrored group: their lobes
    build a frame around a normal the chain has flipped), glossy glass, a point light with a size."""
    import os
    from test_oracle_transforms import family_xml
    text = family_xml(label)[0].replace("@DIR@", str(d))
    for old, new in (('<reflection value="0.8"/>', '<reflection value="0.8" glossiness="0.1"/>'), ('<reflection value="0.2"/>', '<reflection value="0.2" glossiness="0.03"/>'),
                     ('<refraction index="1.5" value="0.9"/>', '<refraction index="1.5" value="0.9" glossiness="0.05"/>'),
                     ('<light type="point" name="key">', '<light type="point" name="key"><size value="2"/>')):
        assert old in text
        text = text.replace(old, new)
    path = os.path.join(str(d), label + "_stochastic.xml")
    with open(path, "w") as f:
        f.write(text)
    return pkg.Scene.from_xml(path)


@pytest.mark.parametrize("gather", [0, 4])
@pytest.mark.parametrize("label", ["T1", "T2"])
def test_sampled_frames(pkg, orc, ctx, xf_dir, label, gather):  # noqa: F811
    """Recipe S at 3 samples (the bar of test_random_scene_sampled: 3e-4) and recipe P at 2 samples (check_paths), on the keyed sample
    streams; the fast variant equals the counting variant bit for bit in every form of recipe W's test."""
    scene = stochastic(pkg, xf_dir, label)
    ctx.upload(scene)
    cam, spp = scene.desc.camera, 2 if gather else 3
    cpu, cst = (orc.render_paths if gather else orc.render_samples)(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
    if gather:  # (the fast variant first: it sizes the frame records the counting variant of recipe P needs)
        ctx.render(pkg.frame_setup(cam, W, H, samples=spp, gather_bounces=gather))
    cnt, gst = ctx.render(pkg.frame_setup(cam, W, H, collect_stats=True, samples=spp, gather_bounces=gather), stats=True)
    fig = {"counting z != oracle": differing(cnt[..., 3].reshape(-1), cpu[..., 3].reshape(-1)), "counters != oracle": int(gst != cst)}
    fast_figures(pkg, ctx, fig, cnt, lambda: pkg.frame_setup(cam, W, H, samples=spp, gather_bounces=gather), (0, 64))
    print("%s recipe %s, %d samples: %s" % (label, "P" if gather else "S", spp, fig))
    settle(orc, [fig], [])
    if gather:
        check_paths(cnt, cpu, orc, "%s recipe P" % label)
    else:
        check_against(cnt, cpu, orc, rel_tol=3e-4)


# ---- updates -----------------------------------------------------------------------------------------------------------------------
def moved_to(pkg, scene, other):
    """A copy of `scene` with every node where `other` (the same scene under other transformations) has it."""
    out = clone(pkg, scene)
    assert out.desc.n_nodes == other.desc.n_nodes
    for i in range(out.desc.n_nodes):
        assert nodes(out)[i].obj_type == nodes(other)[i].obj_type
        for f in ("tm", "itm", "pos"):
            for k in range(len(getattr(nodes(out)[i], f))):
                getattr(nodes(out)[i], f)[k] = getattr(nodes(other)[i], f)[k]
    return out


def update_pair(pkg, d, target):
    """-> (the benign scene: scale +1, aspect 1; the target). "... appended": the target is the benign scene with one more scale on
    every node under the class, through Scene.node_scale (a mirror, or a hundredfold squeeze AFTER the node's rotation: a shear)."""
    name = target.split()[0]
    if name == "T5":
        benign, n_plain = load(pkg, d, "T5", aspect=1.0, file="t5_benign.xml")
        return benign, moved_to(pkg, benign, load(pkg, d, "T5", aspect=t5_aspect(pkg, d, 1.1), file="t5_target.xml")[0])
    benign, n_plain = load(pkg, d, name, benign=True, file=name + "_benign.xml")
    if not target.endswith("appended"):
        return benign, moved_to(pkg, benign, load(pkg, d, name)[0])
    out = clone(pkg, benign)
    for k in transformed(out, n_plain):
        if nodes(out)[k].parent == 0:  # (a child follows its group)
            out.node_scale(k, *((-1.0, 1.0, 1.0) if name == "T1" else (1.0, 1.0, 0.01)))
    for k in range(out.desc.n_nodes):
        if nodes(out)[k].obj_type == 0 and nodes(out)[k].parent == 0:
            out.node_scale(k, *((1.0, -1.0, 1.0) if name == "T1" else (1.0, 0.01, 1.0)))
    return benign, out


@pytest.mark.parametrize("target", ["T1", "T2", "T5 above", "T1 appended", "T2 appended"])
def test_updates_from_a_benign_scene_and_back(pkg, orc, xf_dir, target):  # noqa: F811
    """The updated context renders the image of a fresh upload, bit for bit; its ray-sort box and every occluder list equal the fresh
    upload's and the host builder's (assert_lists_equal: also which lists are dropped); the counting variant equals the oracle; the
    update back to the benign scene restores the first image's bits."""
    benign, moved = update_pair(pkg, xf_dir, target)
    old, new = pkg.Context(0), pkg.Context(0)
    try:
        old.upload(benign)
        first = old.render(frame_of(pkg, benign, W, H))[0]
        usable0 = assert_lists_equal(pkg, old, benign, target + " benign")
        old.update(moved)
        new.upload(moved)
        a, b = old.render(frame_of(pkg, moved, W, H))[0], new.render(frame_of(pkg, moved, W, H))[0]
        fig = {"updated != uploaded": differing(a.reshape(-1, 4), b.reshape(-1, 4)), "updated == benign": int(same_bits(a, first)),
               "sort box differs": int(not same_bits(old.ray_sort_box(), new.ray_sort_box()))}
        cpu, cst = orc.render(moved, W, H, threads=8)
        cnt, gst = old.render(pkg.frame_setup(moved.desc.camera, W, H, collect_stats=True), stats=True)
        fig["counting != fast"] = differing(cnt.reshape(-1, 4), a.reshape(-1, 4))
        fig["counters != oracle"] = int(gst != cst)
        usable = [assert_lists_equal(pkg, c, moved, "%s %s" % (target, what)) for c, what in ((old, "updated"), (new, "uploaded"))]
        old.update(benign)
        back = old.render(frame_of(pkg, benign, W, H))[0]
        fig["back != first"] = differing(back.reshape(-1, 4), first.reshape(-1, 4))
        print("%s: %s; usable lists benign %d, updated %d, uploaded %d" % (target, fig, usable0, usable[0], usable[1]))
        assert usable[0] == usable[1] and assert_lists_equal(pkg, old, benign, target + " back") == usable0
        settle(orc, [fig], [(cnt, cpu)], rel_tol=REL_TOL)
    finally:
        old.close()
        new.close()


# ---- three frames in flight --------------------------------------------------------------------------------------------------------
def test_three_cameras_of_t2_in_flight(pkg, orc, ctx, xf_dir):  # noqa: F811
    scene, _ = scene_of(pkg, xf_dir, "T2")
    ctx.upload(scene)
    cams = []
    for i in range(3):
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        cam.pos[0] += 4.0 * i - 3.0
        cam.pos[2] += 2.0 * i
        cams.append(cam)
    singles = [ctx.render(pkg.frame_setup(c, W, H))[0] for c in cams]
    d = pkg.hip.rtu_device_alloc(ctx._h, 3 * W * H * 16)
    try:
        ctx.render_frames_device([pkg.frame_setup(c, W, H) for c in cams], d)
        ctx.frame_status()
        got = np.empty((3, H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)
    bad = [differing(got[i].reshape(-1, 4), singles[i].reshape(-1, 4)) for i in range(3)]
    print("T2: frames in flight differ from single frames at %s pixels" % bad)
    assert not any(bad)
    assert not same_bits(got[0], got[1]) and not same_bits(got[1], got[2])
    import ctypes
    for i in (0, 2):
        other = clone(pkg, scene)
        ctypes.memmove(ctypes.addressof(other.desc.camera), ctypes.addressof(cams[i]), ctypes.sizeof(cams[i]))
        check_against(got[i], orc.render(other, W, H, threads=8)[0], orc, rel_tol=REL_TOL)
