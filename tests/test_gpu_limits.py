"""GPU: the fixed limits of the device path (rtu_device.h, include/rtu_scene.h), on both sides of each boundary, against the
CPU oracle. Where the path switches strategy the image must not change; where it refuses, the refusal is an error code and
the context renders the next valid scene.

- RTU_MAX_COVER 8 mesh nodes and RTU_MAX_PCOVER 8 plane nodes get a coverage mask for primary rays; only the first 64 scene
  nodes are considered;
- RTU_LMASK_LIGHTS 4 non-ambient lights get occluder lists for their shadow rays;
- RTU_MAX_SHADOW_LIGHTS 13 non-ambient lights fit a ray id; 14 are RTU_ERR_UNSUPPORTED;
- RTU_MAX_NODE_DEPTH 8 (root = depth 0): depth 7 renders, depth 8 is RTU_ERR_UNSUPPORTED;
- coverage masks only while ceil(tiles / 32) <= 12288 words: 5016x5016 with masks, 5024x5024 without.

Each scene: the counting variant against the oracle (z bit-exact, RGB within the bar, counters equal), the fast variant with
a cooperative and a one-lane-per-ray stage 2 bit for bit the same, and a 4-frame batch of nearby cameras against the oracle."""
import math

import numpy as np
import pytest

from bench import orbit_camera
from test_gpu_parity import _write_uv_mesh, check_against

pytestmark = pytest.mark.gpu

OT = 16  # oracle threads
RTU_OBJ_PLANE, RTU_OBJ_TRIMESH = 2, 3  # include/rtu_scene.h
W, H = 160, 120


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def assets(tmp_path_factory):
    d = tmp_path_factory.mktemp("limits")

    def torus(u, v):
        a, b = 2 * math.pi * u, 2 * math.pi * v
        return ((1 + 0.4 * math.cos(b)) * math.cos(a), (1 + 0.4 * math.cos(b)) * math.sin(a), 0.4 * math.sin(b))

    def blob(u, v):
        a, b = 2 * math.pi * u, math.pi * (v - 0.5)
        r = 1.0 + 0.2 * math.sin(5 * a) * math.cos(3 * b)
        return (r * math.cos(b) * math.cos(a), r * math.cos(b) * math.sin(a), r * math.sin(b))
    _write_uv_mesh(d / "torus.obj", 24, 10, torus)
    _write_uv_mesh(d / "blob.obj", 20, 10, blob)
    return d


MATERIALS = """
  <material type="blinn" name="matte"><diffuse r="0.7" g="0.5" b="0.3"/><specular value="0.4"/><glossiness value="20"/></material>
  <material type="blinn" name="matte2"><diffuse r="0.2" g="0.6" b="0.7"/><specular value="0.6"/><glossiness value="60"/></material>
  <material type="blinn" name="floor"><diffuse r="0.5" g="0.5" b="0.5"/><specular value="0.1"/><glossiness value="5"/></material>
  <material type="blinn" name="mirror"><diffuse r="0.1" g="0.1" b="0.15"/><specular value="0.8"/><glossiness value="80"/><reflection value="0.6"/></material>"""
CAMERA = ('<camera><position x="2" y="-17" z="10"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="45"/>'
          '<width value="%d"/><height value="%d"/></camera>' % (W, H))


def lights_xml(n):
    """An ambient light and n non-ambient ones, point and direct alternating, spread over the sky."""
    out = '<light type="ambient" name="amb"><intensity value="0.1"/></light>'
    for i in range(n):
        a = 2 * math.pi * i / max(n, 1)
        k = 0.9 / n
        if i % 2 == 0:
            out += '<light type="point" name="p%d"><intensity value="%r"/><position x="%r" y="%r" z="%r"/></light>' % (
                i, k, 12 * math.cos(a), 12 * math.sin(a), 9 + i % 3)
        else:
            out += '<light type="direct" name="d%d"><intensity value="%r"/><direction x="%r" y="%r" z="-1"/></light>' % (
                i, k, 0.6 * math.cos(a), 0.6 * math.sin(a))
    return out


def mesh(d, name, mat, x, y, z=0.0, s=1.0, rot=0.0):
    return '<object type="obj" name="%s/%s.obj" material="%s"><scale value="%r"/><rotate angle="%r" z="1"/><translate x="%r" y="%r" z="%r"/></object>' % (
        d, name, mat, s, rot, x, y, z)


def sphere(mat, x, y, z, s):
    return '<object type="sphere" name="s" material="%s"><scale value="%r"/><translate x="%r" y="%r" z="%r"/></object>' % (mat, s, x, y, z)


def plane(mat, x, y, z, s, rx=0.0):
    return '<object type="plane" name="pl" material="%s"><scale value="%r"/><rotate angle="%r" x="1"/><translate x="%r" y="%r" z="%r"/></object>' % (
        mat, s, rx, x, y, z)


FLOOR = '<object type="plane" name="floor" material="floor"><scale value="30"/><translate z="-1.5"/></object>'


def write_scene(pkg, d, name, objects, n_lights=2):
    xml = d / (name + ".xml")
    xml.write_text("<xml><scene>%s%s%s</scene>%s</xml>" % (objects, MATERIALS, lights_xml(n_lights), CAMERA))
    return pkg.Scene.from_xml(str(xml))


def grid(n, cols=3, step=3.2):
    for i in range(n):
        yield (i % cols - (cols - 1) / 2) * step, (i // cols - (n - 1) // cols / 2) * step


def check_scene(pkg, orc, ctx, scene):
    """The counting variant, the fast variant with both stage-2 forms and a 4-frame batch of nearby cameras against the oracle."""
    ctx.upload(scene)
    cam0 = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
    cpu, cst = orc.render(scene, W, H, threads=OT)
    cnt, gst = ctx.render(pkg.frame_setup(cam0, W, H, collect_stats=True), stats=True)
    check_against(cnt, cpu, orc)
    assert gst == cst, "counters differ"
    assert gst["primary_hits"] > W * H // 8
    for thr in (1, 10 ** 9):
        fr = pkg.frame_setup(cam0, W, H)
        fr.coop_threshold = thr
        fast, _ = ctx.render(fr)
        assert np.array_equal(fast.view(np.uint32), cnt.view(np.uint32)), "fast (threshold %d) and counting variants differ" % thr
    cams = [orbit_camera(cam0, 4.0 * j) for j in range(4)]
    d = pkg.hip.rtu_device_alloc(ctx._h, len(cams) * W * H * 16)
    try:
        for attempt in range(8):
            ctx.render_frames_device([pkg.frame_setup(c, W, H) for c in cams], d, None)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as e:
                if e.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                    raise
        got = np.empty((len(cams), H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)
    assert np.array_equal(got[0].view(np.uint32), cnt.view(np.uint32)), "batch frame 0 differs from the single frame"
    for j in range(1, len(cams)):
        scene.desc.camera = cams[j]
        try:
            ref, _ = orc.render(scene, W, H, threads=OT)
        finally:
            scene.desc.camera = cam0
        try:
            check_against(got[j], ref, orc)
        except AssertionError as e:
            raise AssertionError("batch frame %d: %s" % (j, e))
    return cnt


def node_field(scene, offset):
    """One int32 field of every scene-graph node (RtuNode, include/rtu_scene.h: 128 bytes; obj_type at byte 88, depth at 100)."""
    import ctypes
    base = scene.desc.nodes
    return [ctypes.c_int32.from_address(base + 128 * i + offset).value for i in range(scene.desc.n_nodes)]


def count_type(pkg, scene, obj_type):
    return sum(1 for t in node_field(scene, 88) if t == obj_type)


@pytest.mark.parametrize("n", [8, 9])
def test_mesh_nodes_around_the_cover_limit(pkg, orc, ctx, assets, n):
    """RTU_MAX_COVER: 8 mesh nodes all get a coverage mask, the 9th goes without; two meshes instanced, a mirror sphere."""
    objs = FLOOR + sphere("mirror", 0, 7, 1, 1.5)
    for i, (x, y) in enumerate(grid(n)):
        objs += mesh(assets, "torus" if i % 2 else "blob", "matte" if i % 3 else "matte2", x, y, 0.0, 1.0, 17.0 * i)
    scene = write_scene(pkg, assets, "mesh%d" % n, objs)
    assert scene.desc.n_meshes == 2 and count_type(pkg, scene, RTU_OBJ_TRIMESH) == n
    check_scene(pkg, orc, ctx, scene)


@pytest.mark.parametrize("n", [8, 9])
def test_plane_nodes_around_the_cover_limit(pkg, orc, ctx, assets, n):
    """RTU_MAX_PCOVER: 8 plane nodes all get a coverage mask, the 9th goes without (tiles, some tilted, and a mirror sphere)."""
    objs = sphere("mirror", 0, 6, 1, 1.5) + mesh(assets, "torus", "matte", 5, 5, 0.5)
    for i, (x, y) in enumerate(grid(n)):
        objs += plane("mirror" if i == 4 else ("matte" if i % 2 else "matte2"), x, y, -1.0 + 0.1 * i, 1.55, 25.0 * (i % 3))
    scene = write_scene(pkg, assets, "plane%d" % n, objs)
    assert count_type(pkg, scene, RTU_OBJ_PLANE) == n
    check_scene(pkg, orc, ctx, scene)


def light_scene(pkg, assets, n):
    objs = FLOOR + sphere("mirror", 0, 4, 1.5, 2.0)
    for i, (x, y) in enumerate(grid(6, cols=3, step=3.5)):
        objs += mesh(assets, "torus" if i % 2 else "blob", "matte" if i % 2 else "matte2", x, y - 2, 0.0, 1.0, 30.0 * i)
    return write_scene(pkg, assets, "lights%d" % n, objs, n_lights=n)


@pytest.mark.parametrize("n", [4, 5, 13])
def test_lights_around_the_occluder_list_and_ray_id_limits(pkg, orc, ctx, assets, n):
    """RTU_LMASK_LIGHTS: the first 4 non-ambient lights get occluder lists, a 5th goes without; 13 lights fill the light bits of a
    ray id (RTU_MAX_SHADOW_LIGHTS), with a mirror so that shadow slots and secondary slots are in use at once."""
    scene = light_scene(pkg, assets, n)
    check_scene(pkg, orc, ctx, scene)
    lights = {l["light"] for l in ctx.light_lists()}
    assert lights == set(range(min(n, 4))), lights


def test_fourteen_lights_are_refused(pkg, orc, ctx, assets):
    """14 non-ambient lights: RTU_ERR_UNSUPPORTED from upload; the context renders the next valid scene."""
    bad = light_scene(pkg, assets, 14)
    assert pkg.hip.rtu_upload_scene(ctx._h, bad.desc_ptr) == pkg.RTU_ERR_UNSUPPORTED
    good = light_scene(pkg, assets, 13)
    ctx.upload(good)
    cpu, _ = orc.render(good, W, H, threads=OT)
    img, _ = ctx.render(pkg.frame_setup(good.desc.camera, W, H))
    check_against(img, cpu, orc)


def nested(assets, depth):
    """Groups nested so that the innermost sphere and mesh are at scene-graph depth `depth` (the root is depth 0)."""
    inner = sphere("mirror", 0, 0, 0, 1.0) + mesh(assets, "torus", "matte", 2.5, 0, 0)
    for k in range(depth - 1):
        inner = '<object name="g%d"><rotate angle="%r" z="1"/><scale value="1.05"/><translate x="%r" y="0.2" z="0.1"/>%s</object>' % (
            k, 7.0 * (k + 1), 0.15 * (k % 3), inner)
    return FLOOR + mesh(assets, "blob", "matte2", -4, 3, 0) + inner


def test_node_depth_limit(pkg, orc, ctx, assets):
    """Depth RTU_MAX_NODE_DEPTH - 1 = 7 renders like the oracle; one deeper is RTU_ERR_UNSUPPORTED and the context renders on."""
    deep = write_scene(pkg, assets, "depth7", nested(assets, 7))
    assert max(node_field(deep, 100)) == 7
    ok = check_scene(pkg, orc, ctx, deep)
    deeper = write_scene(pkg, assets, "depth8", nested(assets, 8))
    assert max(node_field(deeper, 100)) == 8
    assert pkg.hip.rtu_upload_scene(ctx._h, deeper.desc_ptr) == pkg.RTU_ERR_UNSUPPORTED
    ctx.upload(deep)
    img, _ = ctx.render(pkg.frame_setup(deep.desc.camera, W, H))
    assert np.array_equal(img.view(np.uint32), ok.view(np.uint32))


def test_mesh_node_past_the_64th(pkg, orc, ctx, assets):
    """Only the first 64 scene nodes are considered for coverage masks: masked mesh nodes first, 60 spheres, then two mesh nodes
    at indices 64 and 65."""
    objs = mesh(assets, "torus", "matte", -5, 4, 1.0) + mesh(assets, "blob", "matte2", 0, 4, 1.0) + FLOOR
    for i in range(60):
        x, y = (i % 10 - 4.5) * 1.3, (i // 10 - 2.5) * 1.3 - 1
        objs += sphere("mirror" if i % 7 == 0 else "matte2", x, y, -0.9, 0.4)
    objs += mesh(assets, "torus", "matte2", 5, 4, 1.0) + mesh(assets, "blob", "mirror", 5, -5, 1.0)
    scene = write_scene(pkg, assets, "node64", objs)
    assert scene.desc.n_nodes == 1 + 3 + 60 + 2
    types = node_field(scene, 88)
    assert types[1] == types[2] == types[64] == types[65] == RTU_OBJ_TRIMESH
    check_scene(pkg, orc, ctx, scene)


@pytest.mark.parametrize("side", [5016, 5024])
def test_coverage_mask_lds_limit(pkg, orc, ctx, golden, side):
    """teapot2 at 5016x5016 (ceil(627^2 / 32) = 12286 mask words: masks used) and 5024x5024 (12325: no masks). Row bands of each
    against its own oracle: top, middle and the last tile row."""
    words = math.ceil(math.ceil(side / 8) ** 2 / 32)
    assert (words <= 12288) == (side == 5016)
    scene = golden("teapot2_240x135").scene(pkg)
    ctx.upload(scene)
    img, _ = ctx.render(pkg.frame_setup(scene.desc.camera, side, side))
    for row0 in (0, side // 2 - 4, side - 8):
        cpu, _ = orc.render(scene, side, side, threads=OT, row0=row0, nrows=8)
        try:
            check_against(img[row0:row0 + 8], cpu, orc)
        except AssertionError as e:
            raise AssertionError("rows %d-%d: %s" % (row0, row0 + 7, e))
