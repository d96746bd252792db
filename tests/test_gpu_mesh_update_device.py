"""rtu_update_meshes_device: a mesh deformed from DEVICE memory — the vertices come from torch tensors, the reference tree is rebuilt
on the GPU (csrc/rtu_ref_build.hip). Afterwards the context must hold what rtu_scene_set_mesh_vertices + rtu_update_meshes leave
there for the same vertices: the structures are compared with the host restatement by the very assertions of
test_gpu_mesh_update.py, images with a context driven by the host path, counters with the CPU oracle. All comparisons are exact."""
import ctypes

import numpy as np
import pytest

from test_gpu_mesh_update import render
from test_gpu_scene_update import assert_lists_equal, clone, same_bits, torus_scene
from test_mesh_update_host import DEFORMATIONS, assert_same_structures, deform_name, deformed_scene, deformed_vertices
from test_ref_build_host import coincident, deep_row, flat_row, nan_variants, normals_mesh, obj_scene, small_meshes, soup

pytestmark = pytest.mark.gpu

HEADER = ("nv", "nf", "nvn", "nvt", "n_bvh_nodes", "n_elements", "bvh_depth")


def on_device(v):
    import torch
    return torch.from_numpy(np.ascontiguousarray(v, np.float32)).to("cuda:0")


def device_update(ctx, stale, now, meshes, recompute=False, stream=None):
    """The listed meshes of the context take the vertices `now` holds, from torch tensors; the descriptor is `stale` — the host scene
    nobody edited — with the nodes, lights and camera `now` has (here: the same)."""
    import torch
    held = {m: on_device(now.mesh_vertices(m)) for m in meshes}
    torch.cuda.synchronize()
    ctx.update_meshes_device(stale, {m: (t.data_ptr(), None, recompute) for m, t in held.items()}, stream)
    return held


def assert_shape_is(ctx, now, mesh, what):
    got, want = ctx.mesh_shape(mesh), now.mesh(mesh)
    for k in HEADER:
        assert getattr(got, k) == getattr(want, k), "%s: %s is %d, the host's %d" % (what, k, getattr(got, k), getattr(want, k))
    assert bytes(got.bound_min) == bytes(want.bound_min) and bytes(got.bound_max) == bytes(want.bound_max), what + ": bounds differ"
    assert not (got.v or got.f or got.vn or got.fn or got.bvh or got.elements)


def check_structures(pkg, ctx, uploaded, now, meshes, what):
    for m in meshes:
        assert_same_structures(ctx.mesh_arrays(m), pkg.host_mesh(uploaded, m, now), "%s mesh %d" % (what, m), strict_nan=True)
        assert_shape_is(ctx, now, m, what)
    return assert_lists_equal(pkg, ctx, now, what)


def deformed_all(pkg, scene, meshes, d):
    now = clone(pkg, scene)
    for m in meshes:
        now.set_mesh_vertices(m, deformed_vertices(scene, m, d))
    return now


# ---- 1. structures ----------------------------------------------------------------------------------------------------------------

TAGS = ["teapot2_240x135", "torus", "ties"]


def base_scene(pkg, golden, tmp_path, tag):
    from test_ties_host import ties_scene
    scene = torus_scene(pkg, tmp_path) if tag == "torus" else ties_scene(pkg, tmp_path) if tag == "ties" else golden(tag).scene(pkg)
    meshes = list(range(scene.desc.n_meshes))
    assert len(meshes) == (2 if tag == "ties" else 1)
    return scene, meshes


@pytest.mark.parametrize("d", DEFORMATIONS, ids=deform_name)
@pytest.mark.parametrize("tag", TAGS)
def test_structures_equal_the_host_path(pkg, golden, tmp_path, tag, d):
    scene, meshes = base_scene(pkg, golden, tmp_path, tag)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        now = deformed_all(pkg, scene, meshes, d)  # (both meshes of the ties scene in one call)
        device_update(ctx, scene, now, meshes)
        check_structures(pkg, ctx, scene, now, meshes, "%s %s" % (tag, deform_name(d)))
    finally:
        ctx.close()


@pytest.mark.parametrize("tag", TAGS)
def test_a_chain_of_three_and_back(pkg, golden, tmp_path, tag):
    scene, meshes = base_scene(pkg, golden, tmp_path, tag)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        for d in (("twist", 60), ("bulge", None), ("wobble", 2)):
            now = deformed_all(pkg, scene, meshes, d)
            device_update(ctx, scene, now, meshes)
            check_structures(pkg, ctx, scene, now, meshes, "%s chain %s" % (tag, deform_name(d)))
        device_update(ctx, scene, scene, meshes)
        check_structures(pkg, ctx, scene, scene, meshes, tag + " restored")
        for m in meshes:
            assert_same_structures(ctx.mesh_arrays(m), pkg.host_mesh(scene, m), tag + " restored", strict_nan=True)
    finally:
        ctx.close()


def test_small_meshes(pkg, tmp_path):
    ctx = pkg.Context(0)
    try:
        for name, (v, f) in small_meshes().items():
            scene = obj_scene(pkg, tmp_path, name, v, f)
            v2 = coincident(len(f))[0] * np.float32(1.5) if name.startswith("coincident") else soup(len(f), len(f) + 100)[0]
            for vv, what in ((v, name + " as uploaded"), (v2, name + " moved")):
                now = clone(pkg, scene)
                now.set_mesh_vertices(0, vv)
                ctx.upload(scene)
                device_update(ctx, scene, now, [0])
                check_structures(pkg, ctx, scene, now, [0], what)
    finally:
        ctx.close()


def test_nan_vertices(pkg, golden, tmp_path):
    ctx, host = pkg.Context(0), pkg.Context(0)
    try:
        # Tree, element order, boxes, vertices and headers against the host restatement as above. The triangle records
        # of a triangle with a NaN corner are NaN, and WHICH NaN (sign, payload) an operation on a NaN input returns is the
        # processor's choice, not IEEE's: the record kernel of rtu_update_meshes and the x86 restatement differ there, in the host path
        # as well. So against the restatement a NaN equals a NaN, and the bits, NaNs included, are compared with what the host
        # path leaves on the same GPU.
        for tag, scene in (("teapot", golden("teapot2_240x135").scene(pkg)), ("torus", torus_scene(pkg, tmp_path))):
            ctx.upload(scene)
            host.upload(scene)
            for name, v in nan_variants(scene.mesh_vertices(0)).items():
                what = "%s, %s" % (tag, name)
                now = clone(pkg, scene)
                now.set_mesh_vertices(0, v)
                device_update(ctx, scene, now, [0])
                got = ctx.mesh_arrays(0)
                assert_same_structures(got, pkg.host_mesh(scene, 0, now), what, strict_nan=False)
                assert_shape_is(ctx, now, 0, what)
                host.update_meshes(now, [0])
                assert_same_structures(got, host.mesh_arrays(0), what + ", against the host path", strict_nan=True)
    finally:
        ctx.close()
        host.close()


# ---- 2. images --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag,d", [("teapot2_240x135", ("twist", 120)), ("p5_200x150", ("wobble", 1))])
def test_images_equal_the_host_path_and_counters_the_oracle(pkg, orc, golden, tag, d):
    scene = golden(tag).scene(pkg)
    now = deformed_scene(pkg, scene, 0, d)
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        b.upload(scene)
        before, _ = render(pkg, a, scene)
        device_update(a, scene, now, [0])
        b.update_meshes(now, [0])
        ga, _ = render(pkg, a, now)
        gb, _ = render(pkg, b, now)
        assert same_bits(ga, gb), "the device path renders another image than the host path"
        assert not same_bits(ga, before), "the deformation did not change the image"
        W, H = now.desc.camera.img_width, now.desc.camera.img_height
        _, cstats = orc.render(now, W, H, threads=8)
        cnt, gstats = render(pkg, a, now, stats=True)
        assert same_bits(cnt, ga), "fast and counting variants differ"
        assert gstats == cstats, "counters differ from the oracle's: %s vs %s" % (gstats, cstats)  # (they walk the rebuilt tree)
    finally:
        a.close()
        b.close()


def test_recipe_p_frame_equals_the_host_path(pkg, golden):
    scene = golden("teapot1_s2_160x90").scene(pkg)
    now = deformed_scene(pkg, scene, 0, ("wobble", 1))
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        b.upload(scene)
        device_update(a, scene, now, [0])
        b.update_meshes(now, [0])
        pa, _ = render(pkg, a, now, samples=5, gather=4)
        pb, _ = render(pkg, b, now, samples=5, gather=4)
        assert same_bits(pa, pb), "recipe P: the device path renders another image than the host path"
    finally:
        a.close()
        b.close()


# ---- 3. normals -------------------------------------------------------------------------------------------------------------------

def test_recompute_normals(pkg, golden, tmp_path):
    v, f = normals_mesh()
    scene = obj_scene(pkg, tmp_path, "patch", v, f, normals=False)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        for d in (("twist", 60), ("flatten", None), ("wobble", 1)):
            now = deformed_scene(pkg, scene, 0, d)
            now.recompute_normals(0)
            device_update(ctx, scene, now, [0], recompute=True)
            check_structures(pkg, ctx, scene, now, [0], "patch %s, normals recomputed" % deform_name(d))
        # without the flag and without d_vn the normals stay
        kept = ctx.mesh_arrays(0)["vn"]
        now = deformed_scene(pkg, scene, 0, ("bulge", None))
        device_update(ctx, scene, now, [0])
        assert np.array_equal(ctx.mesh_arrays(0)["vn"].view(np.uint32), kept.view(np.uint32))
        # normals handed over
        vn = on_device(np.roll(kept, 1, axis=1))
        t = on_device(now.mesh_vertices(0))
        ctx.update_meshes_device(scene, {0: (t.data_ptr(), vn.data_ptr(), False)})
        assert np.array_equal(ctx.mesh_arrays(0)["vn"].view(np.uint32), np.roll(kept, 1, axis=1).view(np.uint32))
        with pytest.raises(pkg.RtuError) as e:
            ctx.update_meshes_device(scene, {0: (t.data_ptr(), vn.data_ptr(), True)})
        assert e.value.code == pkg.RTU_ERR_ARG
        # the teapot's file carries normals of its own: refused as rtu_scene_recompute_normals refuses
        teapot = golden("teapot2_240x135").scene(pkg)
        assert pkg.host.rtu_scene_recompute_normals(clone(pkg, teapot)._h, 0) == -1
        ctx.upload(teapot)
        held = ctx.mesh_arrays(0)
        t = on_device(teapot.mesh_vertices(0) * np.float32(1.1))
        with pytest.raises(pkg.RtuError) as e:
            ctx.update_meshes_device(teapot, {0: (t.data_ptr(), None, True)})
        assert e.value.code == pkg.RTU_ERR_ARG
        assert_same_structures(ctx.mesh_arrays(0), held, "refused recompute", strict_nan=True)
    finally:
        ctx.close()


# ---- 4. contract ------------------------------------------------------------------------------------------------------------------

def raw_update(pkg, ctx, scene, edits):
    arr = (pkg.RtuMeshDeviceEdit * max(len(edits), 1))()
    for i, (mesh, d_v) in enumerate(edits):
        arr[i].mesh, arr[i].flags, arr[i].d_v, arr[i].d_vn = mesh, 0, d_v, None
    return pkg.hip.rtu_update_meshes_device(ctx._h, scene.desc_ptr, arr, len(edits), None)


def test_a_tree_deeper_than_the_stack_is_refused_after_the_build(pkg, tmp_path):
    fv, ff = flat_row()
    scene = obj_scene(pkg, tmp_path, "flat", fv, ff)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        before, bst = render(pkg, ctx, scene, stats=True)
        held = ctx.mesh_arrays(0)
        t = on_device(deep_row()[0])
        assert raw_update(pkg, ctx, scene, [(0, t.data_ptr())]) == pkg.RTU_ERR_UNSUPPORTED
        assert "depth" in pkg.hip.rtu_last_error(ctx._h).decode()
        after, ast = render(pkg, ctx, scene, stats=True)
        assert same_bits(before, after) and bst == ast, "the refused call changed the image"
        assert_same_structures(ctx.mesh_arrays(0), held, "refused deep row", strict_nan=True)
        assert_shape_is(ctx, scene, 0, "refused deep row")
        # ... and a row that stays within the stack is taken
        v, _ = deep_row(40)
        v = np.concatenate([v, flat_row()[0][120:]])
        now = clone(pkg, scene)
        now.set_mesh_vertices(0, v)
        assert 30 < now.mesh(0).bvh_depth <= 48
        device_update(ctx, scene, now, [0])
        check_structures(pkg, ctx, scene, now, [0], "a row 40 deep")
    finally:
        ctx.close()


def test_refused_calls_leave_the_context_as_it_was(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    now = deformed_scene(pkg, scene, 0, ("twist", 120))
    t = on_device(now.mesh_vertices(0))
    ctx = pkg.Context(0)
    try:
        assert raw_update(pkg, ctx, scene, [(0, t.data_ptr())]) == pkg.RTU_ERR_NO_SCENE
        assert pkg.hip.rtu_context_mesh_shape(ctx._h, 0, ctypes.byref(pkg.RtuMesh())) == pkg.RTU_ERR_NO_SCENE
        ctx.upload(scene)
        before, bst = render(pkg, ctx, scene, stats=True)
        held = ctx.mesh_arrays(0)
        gen_probe = ctx.progressive(pkg.frame_setup(scene.desc.camera, 60, 34, samples=64))
        gen_probe.advance(1)

        def refused(rc, code, what):
            assert rc == code, what
            assert pkg.hip.rtu_last_error(ctx._h).decode(), what
            after, ast = render(pkg, ctx, scene, stats=True)
            assert same_bits(before, after) and bst == ast, what + ": the refused call changed the image"
            assert_same_structures(ctx.mesh_arrays(0), held, what, strict_nan=True)
            gen_probe.advance(1)  # the scene generation did not move

        bad = clone(pkg, scene)
        bad.mesh(0).nv -= 1
        refused(raw_update(pkg, ctx, bad, [(0, t.data_ptr())]), pkg.RTU_ERR_SCENE_SHAPE, "a wrong nv")
        bad = clone(pkg, scene)
        bad.mesh(0).n_elements -= 1
        refused(raw_update(pkg, ctx, bad, [(0, t.data_ptr())]), pkg.RTU_ERR_SCENE_SHAPE, "a wrong n_elements")
        refused(raw_update(pkg, ctx, scene, [(0, t.data_ptr()), (0, t.data_ptr())]), pkg.RTU_ERR_ARG, "a repeated id")
        refused(raw_update(pkg, ctx, scene, [(1, t.data_ptr())]), pkg.RTU_ERR_ARG, "an id out of range")
        refused(raw_update(pkg, ctx, scene, [(0, None)]), pkg.RTU_ERR_ARG, "a NULL d_v")
        refused(pkg.hip.rtu_update_meshes_device(ctx._h, scene.desc_ptr, None, 1, None), pkg.RTU_ERR_ARG, "NULL edits")
        assert pkg.hip.rtu_context_mesh_shape(ctx._h, 1, ctypes.byref(pkg.RtuMesh())) == pkg.RTU_ERR_ARG
        # the descriptor's tree fields of a listed mesh are not read: the host scene is stale by design
        odd = clone(pkg, scene)
        odd.mesh(0).n_bvh_nodes, odd.mesh(0).bvh_depth = 7, 200
        assert raw_update(pkg, ctx, odd, [(0, t.data_ptr())]) == pkg.RTU_OK
        assert_same_structures(ctx.mesh_arrays(0), pkg.host_mesh(scene, 0, now), "a stale descriptor", strict_nan=True)
        # a progressive session of the scene before the update is stale
        with pytest.raises(pkg.RtuError) as e:
            gen_probe.advance(1)
        assert e.value.code == pkg.RTU_ERR_STALE
        gen_probe.close()
        # later updates compare against the mesh as it is now: the header comes from mesh_shape
        assert now.mesh(0).n_bvh_nodes != scene.mesh(0).n_bvh_nodes
        assert pkg.hip.rtu_update_scene(ctx._h, scene.desc_ptr) == pkg.RTU_ERR_SCENE_SHAPE
        assert "n_bvh_nodes" in pkg.hip.rtu_last_error(ctx._h).decode()
        fresh = clone(pkg, scene)
        h, m = ctx.mesh_shape(0), fresh.mesh(0)
        m.n_bvh_nodes, m.bvh_depth = h.n_bvh_nodes, h.bvh_depth
        for k in range(3):
            m.bound_min[k], m.bound_max[k] = h.bound_min[k], h.bound_max[k]
        assert pkg.hip.rtu_update_scene(ctx._h, fresh.desc_ptr) == pkg.RTU_OK
        other = pkg.Context(0)
        try:
            other.upload(now)
            assert same_bits(render(pkg, ctx, now)[0], render(pkg, other, now)[0])
        finally:
            other.close()
    finally:
        ctx.close()


def test_a_chain_allocates_nothing_from_the_second_update_on(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    one, two = deformed_scene(pkg, scene, 0, ("twist", 120)), deformed_scene(pkg, scene, 0, ("twist", 30))
    assert one.mesh(0).n_bvh_nodes < scene.mesh(0).n_bvh_nodes < two.mesh(0).n_bvh_nodes
    t1, t2 = on_device(one.mesh_vertices(0)), on_device(two.mesh_vertices(0))
    ctx, ref = pkg.Context(0), pkg.Context(0)
    try:
        ctx.upload(scene)
        ctx.update_meshes_device(scene, {0: (t1.data_ptr(), None, False)})
        allocs = pkg.hip.rtu_debug_device_allocations()
        for _ in range(5):
            ctx.update_meshes_device(scene, {0: (t2.data_ptr(), None, False)})  # (the first of these grows the tree past the uploaded one)
            ctx.update_meshes_device(scene, {0: (t1.data_ptr(), None, False)})
        ctx.update_meshes_device(scene, {0: (t2.data_ptr(), None, False)})
        grown = pkg.hip.rtu_debug_device_allocations() - allocs
        assert grown == 0, "eleven updates made %d device allocations" % grown
        ref.upload(two)
        assert same_bits(render(pkg, ctx, two)[0], render(pkg, ref, two)[0])
    finally:
        ctx.close()
        ref.close()


def test_vertices_written_on_another_stream(pkg, golden):
    import torch
    scene = golden("teapot2_240x135").scene(pkg)
    now = deformed_scene(pkg, scene, 0, ("bulge", None))
    want = now.mesh_vertices(0)
    half = on_device(want * np.float32(0.5))  # (exact: the product by 2 below gives `want` back bit for bit)
    out = torch.empty_like(half)
    side = torch.cuda.Stream(device="cuda:0")
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            big = torch.randn(2048, 2048, device="cuda:0")
            for _ in range(20):  # work ahead of the write, so that an unordered read would come too early
                big = big @ big * 1e-3
            torch.mul(half, 2.0, out=out)
        ctx.update_meshes_device(scene, {0: (out.data_ptr(), None, False)}, side.cuda_stream)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
        check_structures(pkg, ctx, scene, now, [0], "vertices from a side stream")
    finally:
        ctx.close()


def test_previous_vertices_and_deformed_frames_equal_the_host_path(pkg, golden):
    g = golden("p10_s4_160x120")
    base = g.scene(pkg)
    W, H = 80, 60
    scenes = [base, deformed_scene(pkg, base, 0, ("wobble", 0)), deformed_scene(pkg, base, 0, ("wobble", 1))]
    frame = pkg.frame_setup(base.desc.camera, W, H, samples=2)
    desc = pkg.temporal_desc(W, H)
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        sessions = []
        for ctx in (a, b):
            ctx.keep_previous_vertices(True)
            ctx.upload(base)
            sessions.append(ctx.temporal(desc))
        assert same_bits(sessions[0].frame(frame), sessions[1].frame(frame))
        for k in (1, 2):
            device_update(a, base, scenes[k], [0])
            b.update_meshes(scenes[k], [0])
            motion = pkg.scene_motion(scenes[k - 1], scenes[k], deform_meshes=[0])
            fa, fb = sessions[0].frame_deformed(frame, motion), sessions[1].frame_deformed(frame, motion)
            assert same_bits(fa, fb), "deformed frame %d differs from the host path's" % k
            assert np.array_equal(sessions[0].history(), sessions[1].history())
        assert sessions[0].history().max() >= 2, "no history survived the deformations"
        for s in sessions:
            s.close()
    finally:
        a.close()
        b.close()
