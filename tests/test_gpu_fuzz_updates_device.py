"""rtu_update_meshes_device on the two-mesh random scenes of tests/test_gpu_fuzz_updates.py (instanced meshes under nested non-uniform
scales, lights inside the object box), with what the other tests of the device path never do:

  * edit lists whose position and mesh id differ: mesh 1 alone (slot 0, mesh 1), and both meshes in reverse order;
  * the device path and the host path (rtu_update_meshes, rtu_update_scene) taking turns on one context;
  * previous-generation vertices of a two-mesh scene where one mesh is listed;
  * normals recomputed on the GPU for both random meshes in one call.

After every call: the structures of BOTH meshes equal the host restatement, the occluder lists the host builder's, the image a fresh
upload's bit for bit (fast and counting variants), image and counters the oracle's (the bars of tests/test_gpu_fuzz_updates.py).

The descriptor handed to the device path is a host scene nobody rebuilt: refreshed() gives it the header the context remembers for
every mesh, which is what a caller does who never holds the trees on the host."""
import numpy as np
import pytest

from test_fuzz_host import TWO_MESH_SEEDS, edit_step, mesh_script, w_scene
from test_gpu_fuzz import INSIDE_GLASS_REL_TOL, assets, write_assets  # noqa: F401  (assets: the fixture)
from test_gpu_mesh_update import check_update_against_upload_and_oracle, render
from test_gpu_mesh_update_device import check_structures, on_device, raw_update
from test_gpu_scene_update import same_bits
from test_gpu_temporal import dev
from test_mesh_update_host import assert_same_structures, clone, deformed_scene
from test_ref_build_host import vn_of

pytestmark = pytest.mark.gpu

W, H = 96, 64
PREVIOUS_SEEDS = [3, 15, 18]  # those of test_fuzz_host.py test_mesh_deformations_change_the_image


@pytest.fixture(scope="module")
def pair(pkg):
    a, b = pkg.Context(0), pkg.Context(0)
    yield a, b
    a.close()
    b.close()


def refreshed(pkg, ctx, scene):
    """A clone of `scene` whose meshes carry the header the context remembers (n_bvh_nodes, bvh_depth, bounds): the descriptor of a
    caller whose host scene is stale. Its arrays are still the stale ones; the device path reads none of them."""
    out = clone(pkg, scene)
    for m in range(out.desc.n_meshes):
        h, d = ctx.mesh_shape(m), out.mesh(m)
        d.n_bvh_nodes, d.bvh_depth = h.n_bvh_nodes, h.bvh_depth
        for k in range(3):
            d.bound_min[k], d.bound_max[k] = h.bound_min[k], h.bound_max[k]
    return out


def device_step(pkg, ctx, now, meshes, recompute=False):
    """The listed meshes, in the order given, take the vertices `now` holds from device memory; nodes, lights and camera are those
    of `now`, every mesh header the context's own."""
    import torch
    held = [(m, on_device(now.mesh_vertices(m))) for m in meshes]
    torch.cuda.synchronize()
    ctx.update_meshes_device(refreshed(pkg, ctx, now), {m: (t.data_ptr(), None, recompute) for m, t in held})


def settle(pkg, orc, a, b, scene, now, what):
    """`a` must hold `now`: the structures of both meshes, listed or not (uploaded as `scene`), the lists, the image of a fresh
    upload by `b`, the oracle's image and counters."""
    assert now.desc.camera.img_width == W and now.desc.camera.img_height == H
    check_structures(pkg, a, scene, now, [0, 1], what)
    return check_update_against_upload_and_oracle(pkg, orc, a, b, now, what, shards=False, rel_tol=INSIDE_GLASS_REL_TOL)


def script_by_slot(pkg, scene):
    """mesh_script's three scenes with the edit lists of this file: mesh 0; mesh 1 ALONE (slot 0, mesh 1); both, mesh 1 first."""
    (s0, i0, n0), (s1, i1, n1), (s2, i2, n2) = mesh_script(pkg, scene)
    assert (i0, i1, sorted(i2)) == ([0], [1], [0, 1])
    return [(s0, [0], n0), (s1, [1], n1 + " alone"), (s2, [1, 0], n2 + ", mesh 1 first")]


# ---- 1. the mesh script through the device path ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", TWO_MESH_SEEDS)
def test_mesh_script_through_the_device_path(pkg, orc, pair, assets, seed):  # noqa: F811
    a, b = pair
    scene = w_scene(pkg, assets, seed)
    assert scene.desc.n_meshes == 2
    a.upload(scene)
    for now, ids, name in script_by_slot(pkg, scene):
        device_step(pkg, a, now, ids)
        settle(pkg, orc, a, b, scene, now, "seed %d, %s" % (seed, name))


def test_a_stale_header_of_an_unlisted_mesh_is_refused(pkg, pair, assets):  # noqa: F811
    """Without refreshed(): the second step's descriptor still says how many nodes mesh 0 had when it was uploaded."""
    a, _ = pair
    seed = TWO_MESH_SEEDS[0]
    scene = w_scene(pkg, assets, seed)
    (one, _, _), (two, _, _), _ = script_by_slot(pkg, scene)
    assert one.mesh(0).n_bvh_nodes != scene.mesh(0).n_bvh_nodes  # a property of this input
    a.upload(scene)
    device_step(pkg, a, one, [0])
    held = [a.mesh_arrays(m) for m in (0, 1)]
    before, bst = render(pkg, a, one, stats=True)
    t = on_device(two.mesh_vertices(1))
    assert raw_update(pkg, a, scene, [(1, t.data_ptr())]) == pkg.RTU_ERR_SCENE_SHAPE
    assert "n_bvh_nodes" in pkg.hip.rtu_last_error(a._h).decode()
    for m in (0, 1):
        assert_same_structures(a.mesh_arrays(m), held[m], "refused, mesh %d" % m, strict_nan=True)
    after, ast = render(pkg, a, one, stats=True)
    assert same_bits(before, after) and bst == ast, "the refused call changed the image"
    # ... and with the remembered header the same edit is taken
    assert raw_update(pkg, a, refreshed(pkg, a, scene), [(1, t.data_ptr())]) == pkg.RTU_OK
    check_structures(pkg, a, scene, two, [0, 1], "seed %d, the same edit with the remembered header" % seed)


# ---- 2. the two paths in turn on one context ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", TWO_MESH_SEEDS)
def test_device_and_host_paths_in_turn(pkg, orc, pair, assets, seed):  # noqa: F811
    a, b = pair
    scene = w_scene(pkg, assets, seed)
    (one, _, _), (two, _, _), _ = script_by_slot(pkg, scene)
    what = "seed %d, in turn: " % seed
    a.upload(scene)
    a.update_meshes(one, [0])
    settle(pkg, orc, a, b, scene, one, what + "host, mesh 0")
    device_step(pkg, a, two, [1])
    settle(pkg, orc, a, b, scene, two, what + "device, mesh 1 alone")
    edited = clone(pkg, two)
    edit_step(pkg, edited, np.random.RandomState(9000 + seed))
    a.update(edited)  # (takes `edited`'s headers: the trees the device built have the host's sizes)
    settle(pkg, orc, a, b, scene, edited, what + "a scene edit")
    twisted = deformed_scene(pkg, edited, 0, ("twist", 120))
    device_step(pkg, a, twisted, [0])
    settle(pkg, orc, a, b, scene, twisted, what + "device, mesh 0 twisted")
    last = deformed_scene(pkg, twisted, 1, ("wobble", 1))
    a.update_meshes(last, [1])
    settle(pkg, orc, a, b, scene, last, what + "host, mesh 1")


# ---- 3. previous vertices -------------------------------------------------------------------------------------------------------------

def motion_vectors(pkg, ctx, frame, prev_frame, motion):
    """(hits, surface records, k_motion_vectors_deform's output) of the context's scene through `frame`: the last reads the
    previous generation of vertices the context kept."""
    import torch
    hits, _, surf = ctx.frame_surface(frame)
    d_hits, d_surf, d_tab = dev(hits), dev(surf), dev(motion)
    d_mv = torch.zeros(W * H * 16, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    ctx.motion_vectors_deform_device(pkg.temporal_desc(W, H), prev_frame, d_hits.data_ptr(), d_surf.data_ptr(), d_tab.data_ptr(), len(motion),
                                     d_mv.data_ptr())
    torch.cuda.synchronize()
    return hits, surf, d_mv.cpu().numpy().view(np.float32).reshape(H, W, 4)


@pytest.mark.parametrize("seed", PREVIOUS_SEEDS)
def test_previous_vertices_equal_the_host_path(pkg, assets, seed):  # noqa: F811
    scene = w_scene(pkg, assets, seed)
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        for ctx in (a, b):
            ctx.keep_previous_vertices(True)
            ctx.upload(scene)
        prev, moving = scene, 0
        for now, ids, name in script_by_slot(pkg, scene):
            what = "seed %d, %s" % (seed, name)
            device_step(pkg, a, now, ids)
            b.update_meshes(now, ids)
            motion = pkg.scene_motion(prev, now, deform_meshes=ids)
            frame, prev_frame = pkg.frame_setup(now.desc.camera, W, H), pkg.frame_setup(prev.desc.camera, W, H)
            ha, sa, mva = motion_vectors(pkg, a, frame, prev_frame, motion)
            hb, sb, mvb = motion_vectors(pkg, b, frame, prev_frame, motion)
            assert ha.tobytes() == hb.tobytes() and sa.tobytes() == sb.tobytes(), what + ": hits or surface records differ from the host path's"
            assert same_bits(mva, mvb), what + ": motion vectors differ from the host path's"
            # ... and both are what the host form computes from the previous SCENE
            want = pkg.motion_vectors_deform(prev_frame, ha, sa, prev, motion, W, H)
            assert same_bits(mva, want), what + ": motion vectors differ from the host form's"
            on_listed = np.isin(sa["mesh"], ids)
            moved = on_listed & ((mva.reshape(-1, 4)[:, 0] != 0) | (mva.reshape(-1, 4)[:, 1] != 0))
            print("%s: %d pixels on the listed meshes, %d with a motion vector" % (what, int(on_listed.sum()), int(moved.sum())))
            moving += int(moved.sum())
            prev = now
        assert moving > 0, "no pixel of a deformed mesh moved: the previous vertices were never read"
    finally:
        a.close()
        b.close()


# ---- 4. normals on the random meshes --------------------------------------------------------------------------------------------------

def without_normals(path):
    """The .obj without its vn lines and the normal fields of its faces: the loader computes the normals."""
    out = []
    for line in path.read_text().splitlines():
        w = line.split()
        if w and w[0] == "vn":
            continue
        out.append("f " + " ".join(x.split("/")[0] for x in w[1:]) if w and w[0] == "f" else line)
    path.write_text("\n".join(out) + "\n")


@pytest.fixture(scope="module")
def bare_assets(tmp_path_factory):
    d = write_assets(tmp_path_factory.mktemp("fuzz_bare"))
    without_normals(d / "torus.obj")
    without_normals(d / "blob.obj")
    return d


@pytest.mark.parametrize("seed", PREVIOUS_SEEDS)
def test_normals_of_both_meshes_recomputed_in_reverse_order(pkg, pair, bare_assets, seed):
    a, _ = pair
    scene = w_scene(pkg, bare_assets, seed)
    assert scene.desc.n_meshes == 2 and all(scene.mesh(m).nvn == scene.mesh(m).nv for m in (0, 1))
    now = clone(pkg, script_by_slot(pkg, scene)[-1][0])
    for m in (0, 1):
        now.recompute_normals(m)
        assert not np.array_equal(vn_of(now, m).view(np.uint32), vn_of(scene, m).view(np.uint32))
    a.upload(scene)
    device_step(pkg, a, now, [1, 0], recompute=True)
    what = "seed %d, normals of both recomputed" % seed
    for m in (0, 1):
        got, want = a.mesh_arrays(m)["vn"], vn_of(now, m)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "%s: mesh %d: %d words of vn differ from the host's" % (
            what, m, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    check_structures(pkg, a, scene, now, [0, 1], what)
