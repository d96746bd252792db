"""rtu_update_scene: a scene uploaded once, then moved, relit and re-coloured in place.

The occluder lists it builds on the GPU must equal, entry for entry and bit for bit, the lists the host builder makes from the
edited scene (rtu_debug_light_list, whose lists test_light_lists.py checks ray by ray), and every frame rendered after an update
must equal the frame of a context that uploaded the edited scene afresh."""
import ctypes
import math
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from test_light_lists import RtuLight, RtuNode
from test_scene_update_host import RtuTexture

pytestmark = pytest.mark.gpu


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


def mesh_nodes(scene):
    d = scene.desc
    return [i for i in range(min(d.n_nodes, 64)) if nodes(scene)[i].obj_type == 3][:8]


def shadow_lights(scene):
    return [i for i in range(scene.desc.n_lights) if lights(scene)[i].type != 0]


def clone(pkg, scene):
    return pkg.Scene(pkg.host.rtu_scene_clone(scene.desc_ptr))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def torus_scene(pkg, tmp_path):
    """The instanced-torus scene of test_light_lists.py: nested non-uniform transformations, two nodes of one mesh, a grazing direct
    light, a far point light and one inside the hull (no list from there)."""
    from test_gpu_parity import _write_uv_mesh

    def torus(u, v):
        a, b = 2 * math.pi * u, 2 * math.pi * v
        return ((2 + 0.7 * math.cos(b)) * math.cos(a), (2 + 0.7 * math.cos(b)) * math.sin(a), 0.7 * math.sin(b))
    _write_uv_mesh(tmp_path / "torus.obj", 24, 10, torus)
    xml = tmp_path / "s.xml"
    xml.write_text("""<xml><scene>
      <object name="g"><rotate angle="25" x="1" y="0.3" z="0.2"/><translate x="1" y="-2" z="3"/>
        <object type="obj" name="{o}" material="m"><scale x="1.5" y="0.7" z="2.0"/><rotate angle="40" z="1"/><translate x="-2" z="1"/></object></object>
      <object type="obj" name="{o}" material="m"><scale value="0.8"/><translate x="5" y="3" z="1"/></object>
      <object type="plane" name="floor" material="m"><scale value="30"/><translate z="-4"/></object>
      <material type="blinn" name="m"><diffuse r="0.6" g="0.6" b="0.6"/></material>
      <light type="point" name="far"><intensity value="0.5"/><position x="40" y="-60" z="50"/></light>
      <light type="direct" name="grazing"><intensity value="0.3"/><direction x="1" y="0.2" z="-0.05"/></light>
      <light type="point" name="inside"><intensity value="0.4"/><position x="5" y="3" z="1"/></light>
      <light type="direct" name="down"><intensity value="0.3"/><direction x="0" y="0" z="-1"/></light>
    </scene><camera><position x="0" y="-20" z="6"/><target x="0" y="0" z="1"/><up x="0" y="0" z="1"/><fov value="45"/>
      <width value="64"/><height value="48"/></camera></xml>""".format(o=tmp_path / "torus.obj"))
    return pkg.Scene.from_xml(str(xml))


def assert_lists_equal(pkg, ctx, scene, what=""):
    """Every list the context holds equals the host builder's for the same (light, mesh node), and the context holds a list for
    exactly the pairs the host finds usable."""
    held = {(i["light"], i["cover"]): k for k, i in enumerate(ctx.light_lists())}
    n_light = min(len(shadow_lights(scene)), 4)
    n_cover = len(mesh_nodes(scene))
    usable = 0
    for ls in range(n_light):
        for cs in range(n_cover):
            host = pkg.light_list(scene, ls, cs)
            if host is None:
                assert (ls, cs) not in held, "%s: a list the host finds unusable (light %d, node %d)" % (what, ls, cs)
                continue
            assert (ls, cs) in held, "%s: no list for light %d, node %d" % (what, ls, cs)
            dev = ctx.light_list(held[(ls, cs)])
            usable += 1
            for k in ("G", "point", "node", "light"):
                assert dev[k] == host[k], "%s: %s %s != %s" % (what, k, dev[k], host[k])
            for k in ("X", "Y", "Z", "L"):
                assert same_bits(dev[k].astype(np.float32), host[k].astype(np.float32)), "%s: frame %s differs" % (what, k)
            for k in ("u0", "v0", "su", "sv"):
                assert same_bits(np.float32(dev[k]), np.float32(host[k])), "%s: %s differs" % (what, k)
            assert np.array_equal(dev["cell_off"], host["cell_off"]), "%s: cell offsets differ (light %d, node %d)" % (what, ls, cs)
            assert np.array_equal(dev["entry_face"], host["entry_face"]), "%s: entries differ (light %d, node %d)" % (what, ls, cs)
            assert same_bits(dev["entry_zmin"], host["entry_zmin"]), "%s: zmin bits differ (light %d, node %d)" % (what, ls, cs)
    return usable


def move(pkg, scene, step):
    """One step of an animation: the first shadow light orbits, the first mesh node turns, the first material changes colour."""
    sl = shadow_lights(scene)[0]
    l = lights(scene)[sl]
    nl = RtuLight.from_buffer_copy(bytes(l))
    a = 0.35 * (step + 1)
    if nl.type == 2:
        r = math.hypot(nl.vec[0], nl.vec[1]) or 10.0
        nl.vec[0], nl.vec[1] = r * math.cos(a), r * math.sin(a)
    else:
        nl.vec[0], nl.vec[1], nl.vec[2] = math.cos(a), math.sin(a), -0.8
    scene.set_light(sl, nl)
    scene.node_rotate(mesh_nodes(scene)[0], (0.2, 0.1, 1.0), 9.0)
    if scene.desc.n_materials:
        m = materials(scene)[0]
        m.diffuse[0] = 0.2 + 0.07 * step


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p13_200x150"])
def test_device_lists_equal_host_lists(pkg, golden, tag):
    scene = golden(tag).scene(pkg)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        for step in range(3):
            move(pkg, scene, step)
            ctx.update(scene)
            assert assert_lists_equal(pkg, ctx, scene, "%s step %d" % (tag, step)) >= 1
    finally:
        ctx.close()


def test_device_lists_equal_host_lists_torus(pkg, tmp_path):
    scene = torus_scene(pkg, tmp_path)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        ctx.update(scene)  # the same placement: the device builder's lists for the uploaded scene
        assert assert_lists_equal(pkg, ctx, scene, "torus") >= 6
        assert ctx.light_lists() and all(i["light"] != 2 or i["cover"] != 1 for i in ctx.light_lists())  # inside the hull: none
        rnd = random.Random(5)
        for it in range(50):
            for sl in range(scene.desc.n_lights):
                nl = RtuLight.from_buffer_copy(bytes(lights(scene)[sl]))
                if nl.type == 2:
                    nl.vec[0], nl.vec[1], nl.vec[2] = rnd.uniform(-40, 40), rnd.uniform(-40, 40), rnd.uniform(-10, 40)
                else:
                    nl.vec[0], nl.vec[1], nl.vec[2] = rnd.uniform(-1, 1), rnd.uniform(-1, 1), rnd.uniform(-1, 0.2)
                scene.set_light(sl, nl)
            node = rnd.choice([1, 2, 3])
            scene.node_rotate(node, (rnd.uniform(-1, 1), rnd.uniform(-1, 1), rnd.uniform(-1, 1)), rnd.uniform(-60, 60))
            scene.node_scale(node, rnd.uniform(0.6, 1.5), rnd.uniform(0.6, 1.5), rnd.uniform(0.6, 1.5))
            scene.node_translate(node, (rnd.uniform(-1, 1), rnd.uniform(-1, 1), rnd.uniform(-1, 1)))
            ctx.update(scene)
            assert_lists_equal(pkg, ctx, scene, "torus random %d" % it)
    finally:
        ctx.close()


CHILD = r"""
import sys
sys.path.insert(0, {repo!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as g
import test_gpu_scene_update as t
pkg = g.load_package()
from conftest import Golden
scene = Golden("teapot2_240x135").scene(pkg)
ctx = pkg.Context(0)
ctx.upload(scene)
t.move(pkg, scene, 0)
ctx.update(scene)
assert t.assert_lists_equal(pkg, ctx, scene, "span") == 2
print("G", [i["G"] for i in ctx.light_lists()])
ctx.close()
"""


def test_device_lists_equal_host_lists_at_the_largest_grid(pkg):
    """RTU_LGRID_SPAN high: G starts at its maximum and the halving path runs (the span is read once per process: a child)."""
    env = dict(os.environ, RTU_LGRID_SPAN="400")
    code = CHILD.format(repo=REPO, tests=os.path.join(REPO, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "G [" in r.stdout


def render(pkg, ctx, scene, W, H, samples=0, gather=0):
    f = pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True, samples=samples, gather_bounces=gather)
    return ctx.render(f, stats=True)


@pytest.mark.parametrize("tag,samples,gather", [("teapot2_240x135", 0, 0), ("p7_200x150", 0, 0), ("p11_240x135", 2, 4)])
def test_update_equals_fresh_upload(pkg, golden, tag, samples, gather):
    scene = golden(tag).scene(pkg)
    W, H = scene.desc.camera.img_width, scene.desc.camera.img_height
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        prev = None
        for step in range(8 if samples == 0 else 3):
            move(pkg, scene, step)
            a.update(scene)
            b.upload(scene)
            ga, sa = render(pkg, a, scene, W, H, samples, gather)
            gb, sb = render(pkg, b, scene, W, H, samples, gather)
            assert same_bits(ga, gb), "%s step %d: the updated context renders another image" % (tag, step)
            assert sa == sb, "%s step %d: ray counts differ: %s vs %s" % (tag, step, sa, sb)
            assert prev is None or not same_bits(prev, ga), "the animation did not change the image"
            prev = ga
    finally:
        a.close()
        b.close()


def test_update_equals_fresh_upload_in_a_batch(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    W, H = scene.desc.camera.img_width, scene.desc.camera.img_height
    a, b = pkg.Context(0), pkg.Context(0)
    n = 32
    try:
        a.upload(scene)
        move(pkg, scene, 2)
        a.update(scene)
        b.upload(scene)
        frames = []
        for i in range(n):
            cam = type(scene.desc.camera).from_buffer_copy(bytes(scene.desc.camera))
            cam.pos[0] += 0.21 * i
            frames.append(pkg.frame_setup(cam, W, H))
        got = []
        for ctx in (a, b):
            d = pkg.hip.rtu_device_alloc(ctx._h, n * H * W * 16)
            ctx.render_frames_device(frames, d)
            ctx.frame_status()
            out = np.empty((n, H, W, 4), np.float32)
            assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
            pkg.hip.rtu_device_free(ctx._h, d)
            got.append(out)
        assert same_bits(got[0], got[1])
    finally:
        a.close()
        b.close()


def test_updated_scenes_against_the_oracle(pkg, golden, orc):
    from test_gpu_parity import check_against
    for tag in ("teapot2_240x135", "p7_200x150"):
        scene = golden(tag).scene(pkg)
        scene.set_resolution(96, 64)
        ctx = pkg.Context(0)
        try:
            ctx.upload(scene)
            move(pkg, scene, 4)
            ctx.update(scene)
            gpu, gs = render(pkg, ctx, scene, 96, 64)
            cpu, cs = orc.render(scene, 96, 64, threads=4)
            check_against(gpu, cpu, orc)
            assert gs == cs
        finally:
            ctx.close()


def test_feature_flags_follow_the_update(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    W, H = 120, 68
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scene)
        sl = shadow_lights(scene)[0]
        old = RtuLight.from_buffer_copy(bytes(lights(scene)[sl]))
        soft = RtuLight.from_buffer_copy(bytes(old))
        soft.type, soft.size = 2, 0.5
        scene.set_light(sl, soft)
        a.update(scene)
        with pytest.raises(pkg.RtuError) as e:
            render(pkg, a, scene, W, H)
        assert e.value.code == pkg.RTU_ERR_STOCHASTIC
        scene.set_light(sl, old)
        a.update(scene)
        render(pkg, a, scene, W, H)
        # a reflective mesh material: mesh hits are no longer settled by the lane that found them
        mid = nodes(scene)[mesh_nodes(scene)[0]].material_id
        m = materials(scene)[mid]
        m.reflection[0] = m.reflection[1] = m.reflection[2] = 0.5
        a.update(scene)
        b.upload(scene)
        ga, sa = render(pkg, a, scene, W, H)
        gb, sb = render(pkg, b, scene, W, H)
        assert same_bits(ga, gb) and sa == sb
    finally:
        a.close()
        b.close()


def test_refused_updates_leave_the_context_as_it_was(pkg, golden):
    scene = golden("p7_200x150").scene(pkg)  # textured: texture shapes are checked too
    W, H = 100, 75
    ctx = pkg.Context(0)
    try:
        assert pkg.hip.rtu_update_scene(ctx._h, scene.desc_ptr) == pkg.RTU_ERR_NO_SCENE
        ctx.upload(scene)
        before, bst = render(pkg, ctx, scene, W, H)
        bad = clone(pkg, scene)
        move(pkg, bad, 1)  # placement changes too: none of it may land
        d = bad.desc

        def refuse(mutate, undo):
            mutate()
            assert pkg.hip.rtu_update_scene(ctx._h, bad.desc_ptr) == pkg.RTU_ERR_SCENE_SHAPE
            assert pkg.hip.rtu_last_error(ctx._h).decode()
            undo()
        n = nodes(bad)
        for field in ("parent", "obj_type", "mesh_id", "depth", "subtree_end"):
            i = 1 if field != "parent" else 2
            old = getattr(n[i], field)
            refuse(lambda: setattr(n[i], field, old + 1), lambda: setattr(n[i], field, old))
        meshes = ctypes.cast(d.meshes, ctypes.POINTER(pkg.RtuMesh))
        for field in ("nv", "nf", "nvn", "nvt", "n_bvh_nodes"):
            old = getattr(meshes[0], field)
            refuse(lambda: setattr(meshes[0], field, old + 1), lambda: setattr(meshes[0], field, old))
        tex = ctypes.cast(d.textures, ctypes.POINTER(RtuTexture))
        for field in ("type", "width", "height"):
            old = getattr(tex[1], field)
            refuse(lambda: setattr(tex[1], field, old + 1), lambda: setattr(tex[1], field, old))
        for field in ("n_nodes", "n_meshes", "n_textures", "n_materials"):
            old = getattr(d, field)
            refuse(lambda: setattr(d, field, old - 1), lambda: setattr(d, field, old))
        old_maps = d.material_maps
        refuse(lambda: setattr(d, "material_maps", None), lambda: setattr(d, "material_maps", old_maps))
        # beyond a device limit: what upload returns
        old_mid = n[1].material_id
        n[1].material_id = d.n_materials + 3
        assert pkg.hip.rtu_update_scene(ctx._h, bad.desc_ptr) == pkg.RTU_ERR_ARG
        n[1].material_id = old_mid
        after, ast = render(pkg, ctx, scene, W, H)
        assert same_bits(before, after) and bst == ast
        ctx.update(bad)  # and the fixed scene is taken
        assert not same_bits(before, render(pkg, ctx, bad, W, H)[0])
    finally:
        ctx.close()


def test_update_waits_for_batches_in_flight_and_keeps_memory(pkg, golden):
    import torch
    scene = golden("teapot2_240x135").scene(pkg)
    W, H = scene.desc.camera.img_width, scene.desc.camera.img_height
    old_scene = clone(pkg, scene)
    ctx, ref = pkg.Context(0), pkg.Context(0)
    n = 32
    try:
        ctx.upload(scene)
        frames = [pkg.frame_setup(scene.desc.camera, W, H) for _ in range(n)]
        d = pkg.hip.rtu_device_alloc(ctx._h, n * H * W * 16)
        ctx.render_frames_device(frames, d)  # enqueued, not waited for
        move(pkg, scene, 3)
        ctx.update(scene)
        out = np.empty((n, H, W, 4), np.float32)
        ctx.frame_status()
        assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
        ref.upload(old_scene)
        want_old = render(pkg, ref, old_scene, W, H)[0]
        assert all(same_bits(out[i], want_old) for i in range(n)), "the batch in flight saw the update"
        ctx.render_frames_device(frames, d)
        ctx.frame_status()
        assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
        ref.upload(scene)
        want_new = render(pkg, ref, scene, W, H)[0]
        assert all(same_bits(out[i], want_new) for i in range(n)), "the next batch did not see the update"
        pkg.hip.rtu_device_free(ctx._h, d)
        torch.cuda.init()
        free = []
        for i in range(200):
            move(pkg, scene, i)
            ctx.update(scene)
            if i in (9, 199):
                free.append(torch.cuda.mem_get_info(0)[0])
        assert free[0] - free[1] <= 16 << 20, "updates leak device memory: %d bytes" % (free[0] - free[1])
    finally:
        ctx.close()
        ref.close()


def test_multi_context_update(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    W, H = scene.desc.camera.img_width, scene.desc.camera.img_height
    m, one = pkg.MultiContext([0, 0, 0]), pkg.Context(0)
    try:
        m.upload(scene)
        move(pkg, scene, 5)
        m.update(scene)
        one.upload(scene)
        f = pkg.frame_setup(scene.desc.camera, W, H)
        got = m.render(f)
        want = one.render(f)[0]
        assert same_bits(got, want)
    finally:
        m.close()
        one.close()
