"""rtu_update_meshes: a mesh uploaded once, then deformed in place — new vertices and reference BVH from the host, triangle records and
the boxes of the collapsed fast trees rewritten on the GPU over the kept topology.

Everything the context holds for the mesh afterwards must equal the host restatement (rtu_debug_host_mesh, which
test_mesh_update_host.py checks box by box), and every frame rendered after an update must equal, bit for bit, the frame of a context
that uploaded the deformed scene afresh — and meet the project's bars against the CPU oracle on the deformed scene."""
import ctypes

import numpy as np
import pytest

from test_gpu_scene_update import RtuLight, assert_lists_equal, clone, lights, mesh_nodes, same_bits, shadow_lights, torus_scene
from test_mesh_update_host import (DEFORMATIONS, RENDERED, assert_same_structures, deform_name, deformed_scene, deformed_vertices)

pytestmark = pytest.mark.gpu


def base_scene(pkg, golden, tmp_path, tag):
    return torus_scene(pkg, tmp_path) if tag == "torus" else golden(tag).scene(pkg)


def render(pkg, ctx, scene, stats=False, samples=0, gather=0, shard_count=1):
    W, H = scene.desc.camera.img_width, scene.desc.camera.img_height
    shards, frames, allstats = [], [], None
    for r in range(shard_count):
        fr = pkg.frame_setup(scene.desc.camera, W, H, shard_rank=r, shard_count=shard_count, collect_stats=stats, samples=samples, gather_bounces=gather)
        buf, st = ctx.render(fr, stats=stats)
        shards.append(buf)
        frames.append(fr)
        if stats:
            allstats = st if allstats is None else {k: allstats[k] + st[k] for k in st}
    return pkg.assemble(shards, frames, H), allstats


# ---- 3. structures ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", ["teapot2_240x135", "torus"])
def test_structures_equal_the_host_restatement(pkg, golden, tmp_path, tag):
    scene = base_scene(pkg, golden, tmp_path, tag)
    assert scene.desc.n_meshes == 1 and (tag != "torus" or len(mesh_nodes(scene)) == 2)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        assert_same_structures(ctx.mesh_arrays(0), pkg.host_mesh(scene, 0), tag + " as uploaded", strict_nan=True)
        for d in DEFORMATIONS:
            now = deformed_scene(pkg, scene, 0, d)
            ctx.upload(scene)
            ctx.update_meshes(now, [0])
            what = "%s %s" % (tag, deform_name(d))
            assert_same_structures(ctx.mesh_arrays(0), pkg.host_mesh(scene, 0, now), what, strict_nan=True)
            assert_lists_equal(pkg, ctx, now, what)
        # a chain of updates: the topology stays the uploaded one, everything else is the last mesh's
        ctx.upload(scene)
        for d in (("twist", 60), ("bulge", None), ("wobble", 2)):
            now = deformed_scene(pkg, scene, 0, d)
            ctx.update_meshes(now, [0])
            what = "%s chain %s" % (tag, deform_name(d))
            assert_same_structures(ctx.mesh_arrays(0), pkg.host_mesh(scene, 0, now), what, strict_nan=True)
            assert assert_lists_equal(pkg, ctx, now, what) >= 1
        # back to the uploaded vertices: the uploaded arrays
        ctx.update_meshes(scene, [0])
        assert_same_structures(ctx.mesh_arrays(0), pkg.host_mesh(scene, 0), tag + " restored", strict_nan=True)
        assert_lists_equal(pkg, ctx, scene, tag + " restored")
    finally:
        ctx.close()


# ---- 4. images, recipe W ----------------------------------------------------------------------------------------------------------

def check_update_against_upload_and_oracle(pkg, orc, a, b, now, what, shards=True, rel_tol=None):
    """`a` holds the updated scene, `b` uploads `now` afresh: the same image bit for bit, the project's bars against the oracle, the
    counting variant with the oracle's counters, three shards. rel_tol: the bar of the linear colours, check_against's own if None."""
    from test_gpu_parity import RGB_REL_TOL, check_against
    b.upload(now)
    ga, _ = render(pkg, a, now)
    gb, _ = render(pkg, b, now)
    assert same_bits(ga, gb), what + ": the updated context renders another image than a fresh upload"
    W, H = now.desc.camera.img_width, now.desc.camera.img_height
    cpu, cstats = orc.render(now, W, H, threads=8)
    with np.errstate(invalid="ignore"):
        rel = np.abs(ga[..., :3].astype(np.float64) - cpu[..., :3]) / np.maximum(np.abs(cpu[..., :3].astype(np.float64)), 1e-3)
    print("%s: linear RGB differs by at most %.3g of max(|value|, 1e-3)" % (what, np.nanmax(rel) if np.isfinite(rel).any() else 0.0))
    check_against(ga, cpu, orc, rel_tol=RGB_REL_TOL if rel_tol is None else rel_tol)
    cnt, gstats = render(pkg, a, now, stats=True)
    assert same_bits(cnt, ga), what + ": fast and counting variants differ"
    assert gstats == cstats, what + ": counters differ from the oracle's"
    if shards:
        three, _ = render(pkg, a, now, shard_count=3)
        assert same_bits(three, ga), what + ": three shards differ from one"
    return ga


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p13_200x150", "p5_200x150", "torus"])
def test_update_equals_fresh_upload_and_oracle(pkg, orc, golden, tmp_path, tag):
    scene = base_scene(pkg, golden, tmp_path, tag)
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        prev, _ = render(pkg, a, scene)
        for d in RENDERED:
            now = deformed_scene(pkg, scene, 0, d)
            a.update_meshes(now, [0])  # a chain: every update starts from the previous deformation, the topology from the upload
            img = check_update_against_upload_and_oracle(pkg, orc, a, b, now, "%s %s" % (tag, deform_name(d)))
            assert not same_bits(img, prev), "the deformation did not change the image"
            prev = img
    finally:
        a.close()
        b.close()


def test_deformation_with_a_moved_node_and_light(pkg, orc, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        now = deformed_scene(pkg, scene, 0, ("wobble", 1))
        now.node_rotate(mesh_nodes(now)[0], (0.2, 0.1, 1.0), 25.0)
        sl = shadow_lights(now)[0]
        nl = RtuLight.from_buffer_copy(bytes(lights(now)[sl]))
        nl.vec[0], nl.vec[1] = nl.vec[1] + 3.0, nl.vec[0] - 2.0
        now.set_light(sl, nl)
        a.update_meshes(now, [0])
        check_update_against_upload_and_oracle(pkg, orc, a, b, now, "deformed, turned and relit")
        assert assert_lists_equal(pkg, a, now, "deformed, turned and relit") >= 1
    finally:
        a.close()
        b.close()


# ---- 5. images, recipes S and P ---------------------------------------------------------------------------------------------------

def test_sampled_and_paths_after_an_update(pkg, orc, golden):
    from test_gpu_sampled import RGB8_TOL, check
    g = golden("teapot1_s2_160x90")
    scene = g.scene(pkg)
    W, H, spp = g.width, g.height, g.meta["spp"]
    now = deformed_scene(pkg, scene, 0, ("wobble", 1))
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        a.update_meshes(now, [0])
        b.upload(now)
        # recipe S at the golden's sample count
        ga, _ = render(pkg, a, now, samples=spp)
        gb, _ = render(pkg, b, now, samples=spp)
        assert same_bits(ga, gb), "recipe S: the updated context renders another image than a fresh upload"
        cpu, cst = orc.render_samples(now, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
        check(ga, cpu, orc, spp, "recipe S after an update")
        cnt, gst = render(pkg, a, now, samples=spp, stats=True)
        assert same_bits(cnt, ga) and gst == cst, "recipe S: counting variant"
        # recipe P: 5 samples with the gather (test_paths_vs_oracle's pair and bars)
        pa, _ = render(pkg, a, now, samples=5, gather=4)
        pb, _ = render(pkg, b, now, samples=5, gather=4)
        assert same_bits(pa, pb), "recipe P: the updated context renders another image than a fresh upload"
        cpu, cst = orc.render_paths(now, W, H, 5, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
        assert np.array_equal(pa[..., 3].view(np.uint32), cpu[..., 3].view(np.uint32)), "z differs"
        g8, _, gz8 = orc.postprocess(pa)
        c8, _, cz8 = orc.postprocess(cpu)
        assert np.array_equal(gz8, cz8)
        d8 = np.abs(g8.astype(np.int32) - c8.astype(np.int32))
        assert d8.max() <= RGB8_TOL, "8-bit RGB differs by %d levels at %d pixels" % (d8.max(), (d8 > RGB8_TOL).sum())
        d = np.abs(pa[..., :3].astype(np.float64) - cpu[..., :3].astype(np.float64))
        assert (d / np.maximum(np.abs(cpu[..., :3]), 1e-2)).max() < 1e-3
        cnt, gst = render(pkg, a, now, samples=5, gather=4, stats=True)
        assert same_bits(cnt, pa), "recipe P: fast and counting variants differ"
        assert gst == cst, "recipe P: counters differ"
    finally:
        a.close()
        b.close()


# ---- 6. contract ------------------------------------------------------------------------------------------------------------------

def update_code(pkg, ctx, scene, ids):
    arr = (ctypes.c_uint32 * max(len(ids), 1))(*ids)
    return pkg.hip.rtu_update_meshes(ctx._h, scene.desc_ptr, arr, len(ids))


def test_refused_updates_leave_the_context_as_it_was(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    ctx = pkg.Context(0)
    try:
        assert update_code(pkg, ctx, scene, [0]) == pkg.RTU_ERR_NO_SCENE
        ctx.upload(scene)
        before, bst = render(pkg, ctx, scene, stats=True)
        held = ctx.mesh_arrays(0)

        def refused(bad, ids, code, what):
            assert update_code(pkg, ctx, bad, ids) == code, what
            assert pkg.hip.rtu_last_error(ctx._h).decode(), what
            after, ast = render(pkg, ctx, scene, stats=True)
            assert same_bits(before, after) and bst == ast, what + ": the refused call changed the image"
            assert_same_structures(ctx.mesh_arrays(0), held, what, strict_nan=True)

        now = deformed_scene(pkg, scene, 0, ("twist", 120))
        assert now.mesh(0).n_bvh_nodes != scene.mesh(0).n_bvh_nodes
        refused(now, [0, 0], pkg.RTU_ERR_ARG, "a repeated id")
        refused(now, [1], pkg.RTU_ERR_ARG, "an id out of range")
        assert pkg.hip.rtu_update_meshes(ctx._h, now.desc_ptr, None, 1) == pkg.RTU_ERR_ARG
        for field in ("nv", "nf", "nvn", "n_elements"):
            bad = clone(pkg, now)
            m = bad.mesh(0)
            setattr(m, field, getattr(m, field) - 1)
            refused(bad, [0], pkg.RTU_ERR_SCENE_SHAPE, "a changed " + field)
        # what upload checks of the tree a listed mesh brings, with upload's codes
        bad = clone(pkg, now)
        m = bad.mesh(0)
        root = ctypes.cast(m.bvh, ctypes.POINTER(ctypes.c_uint32))
        assert root[8 + 7] == 0  # node 1 is inner: {bmin[3], index, bmax[3], count}
        root[8 + 3] = m.n_bvh_nodes  # its children lie past the end of the tree
        refused(bad, [0], pkg.RTU_ERR_ARG, "a child index out of range")
        assert pkg.hip.rtu_validate_scene(bad.desc_ptr, None, 0) == pkg.RTU_ERR_ARG  # ... which is upload's code for it
        bad = clone(pkg, now)
        bad.mesh(0).bvh_depth = 3
        refused(bad, [0], pkg.RTU_ERR_ARG, "an understated bvh_depth")
        bad = clone(pkg, now)
        bad.mesh(0).bvh_depth = 200
        refused(bad, [0], pkg.RTU_ERR_UNSUPPORTED, "a tree deeper than the walk's stack")
        bad = clone(pkg, now)
        ctypes.cast(bad.mesh(0).elements, ctypes.POINTER(ctypes.c_uint32))[5] = bad.mesh(0).nf
        refused(bad, [0], pkg.RTU_ERR_ARG, "an element id out of range")
        # n_meshes == 0 is rtu_update_scene: the deformed mesh's other n_bvh_nodes breaks the shape rule
        refused(now, [], pkg.RTU_ERR_SCENE_SHAPE, "a changed n_bvh_nodes of an unlisted mesh")

        # the call that succeeds; then the context remembers the mesh as it is NOW
        ctx.update_meshes(now, [0])
        assert not same_bits(before, render(pkg, ctx, now)[0])
        ctx.update(now)
        assert update_code(pkg, ctx, now, []) == pkg.RTU_OK
        assert pkg.hip.rtu_update_scene(ctx._h, scene.desc_ptr) == pkg.RTU_ERR_SCENE_SHAPE  # 4462 against 4606
        assert "n_bvh_nodes" in pkg.hip.rtu_last_error(ctx._h).decode()
        assert (now.mesh(0).n_bvh_nodes, scene.mesh(0).n_bvh_nodes) == (4462, 4606)
        ctx.update_meshes(scene, [0])
        assert same_bits(before, render(pkg, ctx, scene)[0])
    finally:
        ctx.close()


def test_unlisted_mesh_keeps_its_tree_size(pkg, golden, tmp_path):
    """A scene of two meshes: n_bvh_nodes of the LISTED mesh may change, of the other one not."""
    from test_gpu_parity import _write_uv_mesh
    import math

    def torus(u, v):
        a, b = 2 * math.pi * u, 2 * math.pi * v
        return ((2 + 0.7 * math.cos(b)) * math.cos(a), (2 + 0.7 * math.cos(b)) * math.sin(a), 0.7 * math.sin(b))

    def blob(u, v):
        a, b = 2 * math.pi * u, math.pi * (0.02 + 0.96 * v)
        r = 1.5 + 0.3 * math.sin(3 * a) * math.sin(b)
        return (r * math.sin(b) * math.cos(a), r * math.sin(b) * math.sin(a), r * math.cos(b))
    _write_uv_mesh(tmp_path / "torus.obj", 24, 10, torus)
    _write_uv_mesh(tmp_path / "blob.obj", 20, 12, blob)
    xml = tmp_path / "two.xml"
    xml.write_text("""<xml><scene>
      <object type="obj" name="{d}/torus.obj" material="m"><translate x="-2"/></object>
      <object type="obj" name="{d}/blob.obj" material="m"><translate x="3" z="1"/></object>
      <object type="plane" name="floor" material="m"><scale value="30"/><translate z="-3"/></object>
      <material type="blinn" name="m"><diffuse r="0.6" g="0.6" b="0.6"/></material>
      <light type="point" name="p"><intensity value="0.7"/><position x="10" y="-20" z="30"/></light>
    </scene><camera><position x="0" y="-16" z="5"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="45"/>
      <width value="96"/><height value="64"/></camera></xml>""".format(d=tmp_path))
    scene = pkg.Scene.from_xml(str(xml))
    assert scene.desc.n_meshes == 2
    now = clone(pkg, scene)
    for mesh in (0, 1):
        now.set_mesh_vertices(mesh, deformed_vertices(scene, mesh, ("twist", 120)))
        assert now.mesh(mesh).n_bvh_nodes != scene.mesh(mesh).n_bvh_nodes
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        before, _ = render(pkg, a, scene)
        for ids in ([0], [1]):
            assert update_code(pkg, a, now, ids) == pkg.RTU_ERR_SCENE_SHAPE
            assert "n_bvh_nodes" in pkg.hip.rtu_last_error(a._h).decode()
            assert same_bits(before, render(pkg, a, scene)[0])
        a.update_meshes(now, [1, 0])
        b.upload(now)
        assert same_bits(render(pkg, a, now)[0], render(pkg, b, now)[0])
        for mesh in (0, 1):
            assert_same_structures(a.mesh_arrays(mesh), pkg.host_mesh(scene, mesh, now), "mesh %d of two" % mesh, strict_nan=True)
        # one mesh only: the other keeps what it has
        half = clone(pkg, now)
        half.set_mesh_vertices(0, deformed_vertices(scene, 0, ("bulge", None)))
        a.update_meshes(half, [0])
        b.upload(half)
        assert same_bits(render(pkg, a, half)[0], render(pkg, b, half)[0])
    finally:
        a.close()
        b.close()


def test_progressive_session_turns_stale(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        fr = pkg.frame_setup(scene.desc.camera, 120, 68, samples=8)
        sess = ctx.progressive(fr)
        sess.advance(3)
        before, _ = sess.snapshot()
        ctx.update_meshes(deformed_scene(pkg, scene, 0, ("wobble", 0)), [0])
        with pytest.raises(pkg.RtuError) as e:
            sess.advance(1)
        assert e.value.code == pkg.RTU_ERR_STALE
        after, counts = sess.snapshot()
        assert same_bits(after, before) and (counts == 3).all(), "the snapshot changed with the mesh"
        sess.close()
    finally:
        ctx.close()


def test_updates_back_and_forth_allocate_nothing(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    one, two = deformed_scene(pkg, scene, 0, ("twist", 120)), deformed_scene(pkg, scene, 0, ("twist", 30))
    assert one.mesh(0).n_bvh_nodes < scene.mesh(0).n_bvh_nodes < two.mesh(0).n_bvh_nodes  # the second one has to grow the tree's buffer
    ctx, ref = pkg.Context(0), pkg.Context(0)
    try:
        ctx.upload(scene)
        ctx.update_meshes(one, [0])
        ctx.update_meshes(two, [0])  # the first round: every buffer has seen both sizes
        allocs = pkg.hip.rtu_debug_device_allocations()
        for _ in range(10):
            ctx.update_meshes(one, [0])
            ctx.update_meshes(two, [0])
        grown = pkg.hip.rtu_debug_device_allocations() - allocs
        assert grown == 0, "twenty updates made %d device allocations" % grown
        ref.upload(two)
        assert same_bits(render(pkg, ctx, two)[0], render(pkg, ref, two)[0])
    finally:
        ctx.close()
        ref.close()


def test_multi_context_update_meshes(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    W, H = scene.desc.camera.img_width, scene.desc.camera.img_height
    m, one = pkg.MultiContext([0, 0]), pkg.Context(0)
    try:
        m.upload(scene)
        now = deformed_scene(pkg, scene, 0, ("bulge", None))
        m.update_meshes(now, [0])
        one.upload(scene)
        one.update_meshes(now, [0])
        f = pkg.frame_setup(now.desc.camera, W, H)
        assert same_bits(m.render(f), one.render(f)[0])
        with pytest.raises(pkg.RtuError) as e:
            m.update_meshes(now, [0, 0])
        assert e.value.code == pkg.RTU_ERR_ARG
    finally:
        m.close()
        one.close()
