"""Exact ties and flat meshes in every mesh walk, against the oracle (tests/test_ties_host.py pins the oracle's tie order to the
compiled reference on the same scene, and says why these scenes tie exactly).

The image does not depend on the topology of the fast trees because of one mechanism (rtu_intersect.h): tri_hit<TIE> reports a
triangle that passes every test with t bitwise equal to the best hit, the 4-wide walk and the 8-lane walk (also inside its in-leaf
reduction) then redo the ray on the reference's tree, and until then the inflated box tests must not cull the tied triangle's box —
a box without thickness here. Curved meshes practically never tie; these scenes tie at every pixel of a mesh, so a tie missed
between two distant leaves, inside the 8-lane reduction, after a refit over a stale topology, or a tied triangle culled by a box
test changes colours (or, culled before any hit, z) here.

The bars are the project's: z bit-exact, 8-bit RGB within one level, check_against's linear bound, the counting variant's counters
equal to the oracle's; the fast variant equals the counting variant bit for bit in both stage-2 forms."""
import random
import re

import numpy as np
import pytest

from test_gpu_fuzz import _xf
from test_gpu_parity import RGB8_TOL, check_against, render_gpu
from test_gpu_scene_update import assert_lists_equal
from test_mesh_update_host import assert_same_structures
from test_ties_host import TAG, card_and_plane_pixels, pancake, round_vertices, same_bits, ties_scene, welded_vertices, with_vertices

pytestmark = pytest.mark.gpu

FORMS = ((1, "one lane per ray"), (10 ** 9, "eight lanes per ray"))  # coop_threshold of the two stage-2 forms

# the pancake without a transformation of its own and the camera in its plane, on an axis: with an odd resolution the centre row has
# dir.z == 0 exactly in the pancake's object space, and every box of its trees is hit edge-on
FLAT_NODE = ('<rotate angle="25" x="1"/>\n      <translate x="-0.5" y="1.5" z="1.4"/>', "")
EDGE_ON = [FLAT_NODE,
           ('<position x="0" y="-13" z="7"/><target x="0" y="0" z="0.3"/>', '<position x="0" y="-12" z="0"/><target x="0" y="0" z="0"/>'),
           ('<width value="160"/><height value="120"/>', '<width value="161"/><height value="101"/>')]
# a direct light whose direction lies in the pancake's plane and a point light in that plane: the frame of their occluder lists is
# degenerate for that mesh
LIGHTS_IN_PLANE = [FLAT_NODE,
                   ('<position x="-5" y="-9" z="12"/>', '<position x="6" y="-5" z="0"/>'),
                   ('<direction x="0.5" y="0.4" z="-1"/>', '<direction x="1" y="0.3" z="0"/>')]
# test_gpu_fuzz._make_stochastic's attributes: glossy reflection on `shiny`, a point light with a size
STOCHASTIC = [('<reflection value="0.3"/>', '<reflection value="0.3" glossiness="0.1"/>'),
              ('<light type="point" name="key">', '<light type="point" name="key"><size value="2.0"/>')]


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ties(pkg, orc, golden):
    """The golden scene, the oracle's frame and counters (computed once, never changed)."""
    g = golden(TAG)
    scene = g.scene(pkg)
    cpu, cst = orc.render(scene, g.width, g.height, threads=8)
    cpu.setflags(write=False)
    return g, scene, cpu, cst


def fast(pkg, ctx, scene, W, H, thr, **kw):
    """The uploaded scene by the fast variant in one stage-2 form."""
    fr = pkg.frame_setup(scene.desc.camera, W, H, **kw)
    fr.coop_threshold = thr
    return ctx.render(fr)[0]


def check_scene(pkg, orc, ctx, scene, W, H, what, rel_tol=None):
    """test_random_scene's checks on the uploaded scene: counting variant against the oracle (image, counters), fast variant in
    both stage-2 forms equal to the counting variant bit for bit. Returns the counting variant's image."""
    cpu, cst = orc.render(scene, W, H, threads=8)
    cnt, gst = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
    if rel_tol is None:
        check_against(cnt, cpu, orc)
    else:
        check_against(cnt, cpu, orc, rel_tol=rel_tol)
    assert gst == cst, what + ": counters differ from the oracle's"
    for thr, form in FORMS:
        assert same_bits(fast(pkg, ctx, scene, W, H, thr), cnt), "%s: fast (%s) and counting variants differ" % (what, form)
    return cnt


# ---- the golden scene, recipe W ---------------------------------------------------------------------------------------------------

def test_golden_scene(pkg, orc, ctx, ties):
    g, scene, cpu, cst = ties
    W, H = g.width, g.height
    cnt, gst = render_gpu(pkg, ctx, scene, W, H)
    check_against(cnt, cpu, orc)
    assert gst == cst, "counters differ from the oracle's"
    # the compiled reference
    assert same_bits(cnt[..., 3], g.npz["z"])
    assert (gst["primary_hits"], gst["secondary_rays"], gst["shadow_rays"]) == (g.meta["primary_hits"], g.meta["secondary"], g.meta["shadow"])
    g8, _, gz8 = orc.postprocess(cnt)
    assert np.array_equal(gz8, g.npz["zbuffer_u8"])
    assert np.abs(g8.astype(np.int32) - g.npz["result_u8"].astype(np.int32)).max() <= RGB8_TOL
    for thr, form in FORMS:
        assert same_bits(fast(pkg, ctx, scene, W, H, thr), cnt), "fast (%s) and counting variants differ" % form
    three, st3 = render_gpu(pkg, ctx, scene, W, H, shard_count=3)
    assert same_bits(three, cnt) and st3 == gst, "three shards differ from one"
    three, _ = render_gpu(pkg, ctx, scene, W, H, stats=False, shard_count=3)
    assert same_bits(three, cnt), "three shards of the fast variant differ from one"


def test_golden_scene_without_node_bounds_and_with_a_short_stack(pkg, ctx, ties):
    """rtu_debug_node_bounds off, and rtu_debug_walk_stack_limit 3 (stack overflow and ties in one walk): the same bits."""
    g, scene, cpu, _ = ties
    W, H = g.width, g.height
    ctx.upload(scene)
    want = {thr: fast(pkg, ctx, scene, W, H, thr) for thr, _ in FORMS}
    assert same_bits(want[1][..., 3], cpu[..., 3]) and same_bits(want[1], want[10 ** 9])
    try:
        assert pkg.hip.rtu_debug_node_bounds(ctx._h, 0) == 0
        for thr, form in FORMS:
            assert same_bits(fast(pkg, ctx, scene, W, H, thr), want[thr]), "node-level bounds change the image (%s)" % form
        assert pkg.hip.rtu_debug_node_bounds(ctx._h, 1) == 0
        assert pkg.hip.rtu_debug_walk_stack_limit(ctx._h, 3) == 0
        for thr, form in FORMS:
            assert same_bits(fast(pkg, ctx, scene, W, H, thr), want[thr]), "a walk stack of 3 entries changes the image (%s)" % form
    finally:
        pkg.hip.rtu_debug_node_bounds(ctx._h, 1)
        ctx.upload(scene)  # restores the limit


def test_the_tie_mechanism_fires(pkg, ctx, ties):
    """Touched-bytes mode: in EACH stage-2 form walks finish on the reference's tree (inner_ref), after the fast walk of that form ran
    (inner4 / inner8) — the images above are not the work of a path that avoids the fast trees."""
    g, scene, cpu, _ = ties
    W, H = g.width, g.height
    ctx.upload(scene)
    for (thr, form), own in zip(FORMS, ("inner4", "inner8")):
        img = fast(pkg, ctx, scene, W, H, thr, collect_stats=2)
        t = ctx.touched()
        assert same_bits(img[..., 3], cpu[..., 3])
        assert same_bits(img, fast(pkg, ctx, scene, W, H, thr)), "touched-bytes mode changed the image"
        total = {k: sum(c[k] for c in t.values()) for k in ("inner_ref", "inner4", "inner8")}
        print("%s: inner_ref %d, inner4 %d, inner8 %d" % (form, total["inner_ref"], total["inner4"], total["inner8"]))
        assert total["inner_ref"] > 0, "no walk fell back to the reference's tree (%s)" % form
        assert total[own] > 0, "the fast walk of this form did not run (%s)" % form
        stage2 = [c for name, c in t.items() if name.startswith(("k_primary2", "k_trace2"))]
        assert stage2 and sum(c["inner_ref"] for c in stage2) > 0 and sum(c[own] for c in stage2) > 0


def test_both_node_orders_of_the_plane_and_card_tie(pkg, orc, ctx, ties):
    """The oracle shows the card where the card is the earlier node and the plane where the plane is (asserted from its image); the
    device shows the same winners in every form."""
    g, scene, cpu, _ = ties
    W, H = g.width, g.height
    half = W // 2
    yellow, blue = card_and_plane_pixels(cpu[..., :3])
    assert yellow[:, :half].sum() > 500 and yellow[:, half:].sum() == 0 and blue[:, half:].sum() > 1000
    ctx.upload(scene)
    imgs = [ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)[0]] + [fast(pkg, ctx, scene, W, H, thr) for thr, _ in FORMS]
    for img in imgs:
        gy, gb = card_and_plane_pixels(img[..., :3])
        # (a pixel within rounding of a threshold of the masks may differ: none does on these colours)
        assert np.array_equal(gy, yellow) and np.array_equal(gb, blue), "another winner than the oracle's"
        check_against(img, cpu, orc)


def centre_row_dir_z(pkg, scene, W, H):
    """The z of the primary rays of the centre row (recipe W: the pixel's centre, RenderFunctions.cpp:258-268), in binary32; the
    pancake's node has no transformation, so this is the ray's z in its object space."""
    f32 = np.float32
    fr = pkg.frame_setup(scene.desc.camera, W, H)
    z = (f32(fr.origin[2]) + f32(fr.u[2]) * (f32(W // 2) + f32(0.5))) + f32(fr.v[2]) * (f32(H // 2) + f32(0.5))
    return float(z - f32(fr.cam_pos[2]))


# ---- awkward views and lights -----------------------------------------------------------------------------------------------------

def test_edge_on_view(pkg, orc, ctx, tmp_path):
    scene = ties_scene(pkg, tmp_path, EDGE_ON)
    W, H = 161, 101
    assert centre_row_dir_z(pkg, scene, W, H) == 0, "the centre row does not lie in the pancake's plane exactly"
    ctx.upload(scene)
    cnt = check_scene(pkg, orc, ctx, scene, W, H, "edge-on")
    assert (cnt[..., 3] < 1e29).sum() > 5000


def test_lights_in_the_plane_of_the_flat_mesh(pkg, orc, ctx, tmp_path):
    scene = ties_scene(pkg, tmp_path, LIGHTS_IN_PLANE)
    W, H = 160, 120
    ctx.upload(scene)
    assert_lists_equal(pkg, ctx, scene, "lights in the plane, as uploaded")
    a = check_scene(pkg, orc, ctx, scene, W, H, "lights in the plane, as uploaded")
    ctx.update(scene)  # the same scene through the device's list builder
    assert_lists_equal(pkg, ctx, scene, "lights in the plane, after an update")
    b = check_scene(pkg, orc, ctx, scene, W, H, "lights in the plane, after an update")
    assert same_bits(a, b)


# ---- recipes S and P --------------------------------------------------------------------------------------------------------------

def test_sampled_and_paths(pkg, orc, ctx, tmp_path):
    from test_gpu_sampled import check, render_gpu as render_sampled, render_paths_gpu
    scene = ties_scene(pkg, tmp_path, STOCHASTIC)
    W, H, spp = 160, 120, 3
    cpu, cst = orc.render_samples(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
    cnt, gst = render_sampled(pkg, ctx, scene, W, H, spp, stats=True)
    check(cnt, cpu, orc, spp, "recipe S, counting variant")
    assert gst == cst, "recipe S: counters differ from the oracle's"
    for coop in (False, True):
        img, _ = render_sampled(pkg, ctx, scene, W, H, spp, coop=coop)
        assert same_bits(img, cnt), "recipe S: fast (coop %s) and counting variants differ" % coop
    # recipe P at 2 samples, the bars of test_paths_vs_oracle
    cpu, cst = orc.render_paths(scene, W, H, 2, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=8)
    gpu = render_paths_gpu(pkg, ctx, scene, W, H, 2)
    assert same_bits(gpu[..., 3], cpu[..., 3]), "recipe P: z differs"
    g8, _, gz8 = orc.postprocess(gpu)
    c8, _, cz8 = orc.postprocess(cpu)
    assert np.array_equal(gz8, cz8)
    d8 = np.abs(g8.astype(np.int32) - c8.astype(np.int32))
    assert d8.max() <= RGB8_TOL, "recipe P: 8-bit RGB differs by %d levels at %d pixels" % (d8.max(), (d8 > RGB8_TOL).sum())
    d = np.abs(gpu[..., :3].astype(np.float64) - cpu[..., :3].astype(np.float64))
    assert (d / np.maximum(np.abs(cpu[..., :3]), 1e-2)).max() < 1e-3
    frs = pkg.frame_setup(scene.desc.camera, W, H, samples=2, gather_bounces=4, collect_stats=True)
    cnt, gst = ctx.render(frs, stats=True)
    assert same_bits(cnt, gpu), "recipe P: fast and counting variants differ"
    assert gst == cst, "recipe P: counters differ from the oracle's"
    for coop in (False, True):
        assert same_bits(render_paths_gpu(pkg, ctx, scene, W, H, 2, coop=coop), gpu), "recipe P: the stage-2 form changes the image"


# ---- frames in flight -------------------------------------------------------------------------------------------------------------

def test_a_batch_of_frames(pkg, ctx, tmp_path):
    """rtu_render_frames_device with three cameras, one of them edge-on: each frame is its single render, bit for bit."""
    W, H = 161, 101
    size = ('<width value="160"/><height value="120"/>', '<width value="161"/><height value="101"/>')
    scene = ties_scene(pkg, tmp_path, EDGE_ON)
    others = [ties_scene(pkg, tmp_path, [FLAT_NODE, size], "cam1.xml"),
              ties_scene(pkg, tmp_path, [FLAT_NODE, size, ('<position x="0" y="-13" z="7"/>', '<position x="9" y="-8" z="-0.5"/>'), ('<fov value="42"/>', '<fov value="55"/>')],
                         "cam2.xml")]
    cams = [type(s.desc.camera).from_buffer_copy(s.desc.camera) for s in [scene] + others]
    ctx.upload(scene)
    d = pkg.hip.rtu_device_alloc(ctx._h, 3 * W * H * 16)
    try:
        for thr, form in FORMS:
            frames = [pkg.frame_setup(c, W, H) for c in cams]
            for f in frames:
                f.coop_threshold = thr
            singles = [ctx.render(f)[0] for f in frames]
            assert not same_bits(singles[0], singles[1]) and not same_bits(singles[1], singles[2])
            for stats in (0, 1):
                for f in frames:
                    f.collect_stats = stats
                ctx.render_frames_device(frames, d)
                ctx.frame_status()
                got = np.empty((3, H, W, 4), np.float32)
                assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
                for i in range(3):
                    assert same_bits(got[i], singles[i]), "frame %d of the batch differs from its single render (%s, stats %d)" % (i, form, stats)
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)


# ---- rtu_update_meshes over a stale topology --------------------------------------------------------------------------------------

def check_step(pkg, orc, a, b, uploaded, now, mesh, what):
    """After a.update_meshes(now): the bits of a fresh upload, the oracle, its counters, three shards
    (check_update_against_upload_and_oracle), both stage-2 forms, and the structures of the host restatement."""
    from test_gpu_mesh_update import check_update_against_upload_and_oracle
    img = check_update_against_upload_and_oracle(pkg, orc, a, b, now, what)
    W, H = now.desc.camera.img_width, now.desc.camera.img_height
    for thr, form in FORMS:
        assert same_bits(fast(pkg, a, now, W, H, thr), img), "%s: the updated context, %s" % (what, form)
        assert same_bits(fast(pkg, b, now, W, H, thr), img), "%s: the fresh upload, %s" % (what, form)
    assert_same_structures(a.mesh_arrays(mesh), pkg.host_mesh(uploaded, mesh, now), what, strict_nan=True)
    assert_lists_equal(pkg, a, now, what)
    return img


@pytest.fixture(scope="module")
def shapes(pkg, tmp_path_factory):
    """The ties scene with the pancake flat (as its file has it), round (the torus it was pressed from) and half-welded."""
    flat = ties_scene(pkg, tmp_path_factory.mktemp("shapes"))
    mesh = pancake(flat)
    v = flat.mesh_vertices(mesh)
    return mesh, {"flat": flat, "round": with_vertices(pkg, flat, mesh, round_vertices(v)), "welded": with_vertices(pkg, flat, mesh, welded_vertices(v))}


@pytest.mark.parametrize("chain", [("round", "flat"), ("flat", "round"), ("round", "flat", "round"), ("flat", "welded"), ("round", "welded", "flat")],
                         ids="-".join)
def test_update_meshes_over_a_stale_topology(pkg, orc, shapes, chain):
    """The first shape is uploaded, the others follow by rtu_update_meshes on the same context: the topology of the fast trees stays
    the first shape's however far the mesh has moved. (An upload of the welded pancake is the `b` context of the check.)"""
    mesh, scenes = shapes
    a, b = pkg.Context(0), pkg.Context(0)
    try:
        a.upload(scenes[chain[0]])
        prev = None
        for name in chain[1:]:
            a.update_meshes(scenes[name], [mesh])
            img = check_step(pkg, orc, a, b, scenes[chain[0]], scenes[name], mesh, "%s -> %s" % (chain[0], name))
            assert prev is None or not same_bits(img, prev), "the deformation did not change the image"
            prev = img
    finally:
        a.close()
        b.close()


# ---- tie fuzz ---------------------------------------------------------------------------------------------------------------------

def _write_soup(path, rnd):
    """2 to 4 coincident layers of 30 to 120 random triangles each in one random object-space axis plane, a normal per layer; a random
    third of the faces present twice, the copy with another normal; vt present; faces shuffled."""
    axis, c = rnd.randrange(3), rnd.choice([0.0, rnd.uniform(-1, 1)])
    verts, uvs, norms, faces = [], [], [], []

    def unit():
        n = [rnd.uniform(-1, 1) for _ in range(3)]
        n[axis] = rnd.choice([-1, 1]) * (1.0 + abs(n[axis]))
        ln = sum(x * x for x in n) ** 0.5
        return tuple(x / ln for x in n)
    for layer in range(rnd.randrange(2, 5)):
        norms.append(unit())
        for _ in range(rnd.randrange(30, 121)):
            cx, cy = rnd.uniform(-2, 2), rnd.uniform(-2, 2)
            tri = []
            for _ in range(3):
                p = [cx + rnd.uniform(-0.9, 0.9), cy + rnd.uniform(-0.9, 0.9)]
                p.insert(axis, c)
                verts.append(tuple(p))
                uvs.append((rnd.random(), rnd.random()))
                tri.append(len(verts))
            faces.append((tri, len(norms)))
    norms.append(unit())
    faces += [(tri, len(norms)) for tri, _ in rnd.sample(faces, len(faces) // 3)]
    rnd.shuffle(faces)
    with open(path, "w") as f:
        for v in verts: f.write("v %r %r %r\n" % v)
        for t in uvs: f.write("vt %r %r\n" % t)
        for n in norms: f.write("vn %r %r %r\n" % n)
        for tri, n in faces: f.write("f " + " ".join("%d/%d/%d" % (k, k, n) for k in tri) + "\n")


def tie_fuzz_scene(pkg, d, seed):
    """Two soups under test_gpu_fuzz's random nested transformations, one of them instanced twice, materials alternating mirror /
    matte; a mirror floor, a sphere, random lights and camera. Returns (scene, the same scene without its meshes)."""
    import math
    rnd = random.Random(4000 + seed)
    for name in "ab":
        _write_soup(d / ("%s%d.obj" % (name, seed)), rnd)
    soup = lambda name, mat: '<object type="obj" name="%s/%s%d.obj" material="%s">%s</object>' % (d, name, seed, mat, _xf(rnd))
    objs = '<object name="g1">%s%s<object name="g2">%s%s</object></object>' % (_xf(rnd, scale=False), soup("a", "mirror"), _xf(rnd), soup("b", "matte"))
    objs += '<object name="g3">%s%s</object>' % (_xf(rnd, scale=False), soup("a", "matte"))
    objs += soup("b", "mirror")
    objs += '<object type="sphere" name="ball" material="mirror">%s</object>' % _xf(rnd)
    objs += '<object type="plane" name="floor" material="mirror"><scale value="40"/><translate z="-5"/></object>'
    mats = ('<material type="blinn" name="mirror"><diffuse r="%r" g="%r" b="%r"/><specular value="%r"/><glossiness value="%r"/><reflection value="%r"/></material>'
            '<material type="blinn" name="matte"><diffuse r="%r" g="%r" b="%r"/><specular value="%r"/><glossiness value="%r"/></material>') % (
        rnd.random(), rnd.random(), rnd.random(), rnd.uniform(0, 0.9), rnd.uniform(5, 120), rnd.uniform(0.2, 0.8),
        rnd.random(), rnd.random(), rnd.random(), rnd.uniform(0, 0.9), rnd.uniform(5, 120))
    lights = '<light type="ambient" name="a"><intensity value="%r"/></light>' % rnd.uniform(0.05, 0.3)
    lights += '<light type="direct" name="d"><intensity value="%r"/><direction x="%r" y="%r" z="-1"/></light>' % (rnd.uniform(0.3, 0.8), rnd.uniform(-1, 1), rnd.uniform(-1, 1))
    lights += '<light type="point" name="p"><intensity value="%r"/><position x="%r" y="%r" z="%r"/></light>' % (
        rnd.uniform(0.3, 0.8), rnd.uniform(-10, 10), rnd.uniform(-10, 10), rnd.uniform(5, 15))
    a = rnd.uniform(0, 2 * math.pi)
    cam = ('<camera><position x="%r" y="%r" z="%r"/><target x="%r" y="%r" z="0"/><up x="0" y="0" z="1"/><fov value="%r"/>'
           '<width value="96"/><height value="64"/></camera>') % (16 * math.cos(a), 16 * math.sin(a), rnd.uniform(2, 10), rnd.uniform(-1, 1), rnd.uniform(-1, 1), rnd.uniform(30, 70))
    xml = "<xml><scene>%s%s%s</scene>%s</xml>" % (objs, mats, lights, cam)
    (d / ("t%d.xml" % seed)).write_text(xml)
    (d / ("t%d_bare.xml" % seed)).write_text(re.sub(r'<object type="obj".*?</object>', "", xml))
    return pkg.Scene.from_xml(str(d / ("t%d.xml" % seed))), pkg.Scene.from_xml(str(d / ("t%d_bare.xml" % seed)))


def mesh_hit_pixels(orc, scene, bare, W, H):
    """Pixels whose nearest surface is a mesh: where the oracle's z changes when the meshes are taken out of the scene."""
    z, zb = orc.render(scene, W, H, threads=8)[0][..., 3], orc.render(bare, W, H, threads=8)[0][..., 3]
    return int((z.view(np.uint32) != zb.view(np.uint32)).sum())


# chosen on the CPU among seeds 0..: every one shows at least 50 mesh-hit pixels in the oracle's image (a seed that does not is
# replaced here, not skipped at run time)
TIE_SEEDS = [0, 1, 2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("seed", TIE_SEEDS)
def test_tie_fuzz(pkg, orc, ctx, tmp_path, seed):
    scene, bare = tie_fuzz_scene(pkg, tmp_path, seed)
    W, H = 96, 64
    assert scene.desc.n_meshes == 2
    hit = mesh_hit_pixels(orc, scene, bare, W, H)
    assert hit >= 50, "seed %d shows %d mesh-hit pixels: choose another" % (seed, hit)
    ctx.upload(scene)
    # (test_random_scene's bound on linear RGB: mirrors facing mirrors multiply many powf terms)
    check_scene(pkg, orc, ctx, scene, W, H, "seed %d" % seed, rel_tol=1e-4)
