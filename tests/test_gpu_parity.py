"""GPU parity tests proper: the HIP path, called through the C-ABI, against the CPU
oracle on the same inputs and against the goldens generated from the compiled
reference. Bars: float z bit-exact (hence ZBuffer.png exact), 8-bit RGB
within +-1 per channel (device powf/expf vs glibc), ray / traversal counters equal."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ALL_TAGS, FULL_TAGS, SMALL_TAGS, TEX_TAGS, sha256

pytestmark = pytest.mark.gpu

RGB8_TOL = 1          # levels of 255, BASELINE.md "RGB +-1/255"
RGB_REL_TOL = 2e-5    # linear float RGB: a few ulp through <=6 levels of powf/expf products


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def render_gpu(pkg, ctx, scene, W, H, stats=True, shard_count=1):
    ctx.upload(scene)
    shards, frames, allstats = [], [], None
    for r in range(shard_count):
        fr = pkg.frame_setup(scene.desc.camera, W, H, shard_rank=r, shard_count=shard_count, collect_stats=stats)
        buf, st = ctx.render(fr, stats=stats)
        shards.append(buf)
        frames.append(fr)
        if stats:
            allstats = st if allstats is None else {k: allstats[k] + st[k] for k in st}
    return pkg.assemble(shards, frames, H), allstats


def check_against(gpu, ref_rgbz, orc, rel_tol=RGB_REL_TOL):
    zbad = int((gpu[..., 3].view(np.uint32) != ref_rgbz[..., 3].view(np.uint32)).sum())
    assert zbad == 0, "%d pixels differ in float z" % zbad
    g8, _, gz8 = orc.postprocess(gpu)
    c8, _, cz8 = orc.postprocess(ref_rgbz)
    assert np.array_equal(gz8, cz8), "z-image differs"
    d8 = np.abs(g8.astype(np.int32) - c8.astype(np.int32))
    assert d8.max() <= RGB8_TOL, "8-bit RGB differs by %d levels at %d pixels" % (d8.max(), (d8 > RGB8_TOL).sum())
    a, b = gpu[..., :3].astype(np.float64), ref_rgbz[..., :3].astype(np.float64)
    # the reference's own arithmetic yields NaN colours on some inputs (tests/scenes/multimtl: 1029 pixels); they are
    # results like any other: the same pixels must be NaN on both sides, the rest is compared by value
    nan = np.isnan(b)
    assert np.array_equal(np.isnan(a), nan), "NaN colours at different pixels"
    rel = (np.abs(a - b) / np.maximum(np.abs(b), 1e-3))[~nan]
    assert rel.max() <= rel_tol, "linear RGB relative error %.3g" % rel.max()
    return int((d8 > 0).sum())


@pytest.mark.parametrize("tag", ALL_TAGS)
def test_gpu_vs_oracle_and_golden(pkg, orc, ctx, golden, tag):
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = g.width, g.height
    gpu, gstats = render_gpu(pkg, ctx, scene, W, H)          # counting variant: walks the reference's node set
    fast, _ = render_gpu(pkg, ctx, scene, W, H, stats=False)  # fast variant: culling, any-hit shadows, speculative Fresnel ray
    assert np.array_equal(gpu.view(np.uint32), fast.view(np.uint32)), "fast and counting variants differ"
    cpu, cstats = orc.render(scene, W, H, threads=8)
    nflip = check_against(gpu, cpu, orc)
    assert gstats == cstats, "counters differ"
    # goldens from the compiled reference
    assert sha256(gpu[..., 3]) == g.meta["sha256_z_f32"]
    assert gstats["primary_hits"] == g.meta["primary_hits"]
    assert gstats["secondary_rays"] == g.meta["secondary"]
    assert gstats["shadow_rays"] == g.meta["shadow"]
    g8, _, gz8 = orc.postprocess(gpu)
    assert np.array_equal(gz8, g.npz["zbuffer_u8"]), "ZBuffer image differs from the reference's"
    d = np.abs(g8.astype(np.int32) - g.npz["result_u8"].astype(np.int32))
    assert d.max() <= RGB8_TOL
    print("%s: %d/%d channel values off by one level" % (tag, nflip, W * H * 3))


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p4_240x135"])
@pytest.mark.parametrize("shards", [2, 3, 8, 24])  # 24 > the 17 bands of a 135-row image: some shards are empty
def test_sharded_render_is_identical(pkg, orc, ctx, golden, tag, shards):
    """Band-interleaved shards assemble to exactly the single-GPU image (bit for bit,
    RGB included: same kernel, same arithmetic), for every shard count."""
    g = golden(tag)
    scene = g.scene(pkg)
    one, st1 = render_gpu(pkg, ctx, scene, g.width, g.height)
    many, stn = render_gpu(pkg, ctx, scene, g.width, g.height, shard_count=shards)
    assert np.array_equal(one.view(np.uint32), many.view(np.uint32))
    assert st1 == stn


def test_ragged_resolution(pkg, orc, ctx, golden):
    """Width/height not multiples of the 8x8 tile, and a 1x1 image."""
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    for (W, H) in [(61, 45), (8, 8), (1, 1), (17, 3)]:
        gpu, gst = render_gpu(pkg, ctx, scene, W, H)
        cpu, cst = orc.render(scene, W, H, threads=2)
        check_against(gpu, cpu, orc)
        assert gst == cst


def test_stats_variant_matches_fast_variant(pkg, ctx, golden):
    g = golden("p4_240x135")
    scene = g.scene(pkg)
    a, _ = render_gpu(pkg, ctx, scene, g.width, g.height, stats=True)
    b, _ = render_gpu(pkg, ctx, scene, g.width, g.height, stats=False)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_device_render_and_timing_entry(pkg, ctx, golden):
    """rtu_render_frame_device + rtu_time_render on a caller-owned device buffer."""
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    ctx.upload(scene)
    fr = pkg.frame_setup(scene.desc.camera, g.width, g.height)
    nbytes = g.width * g.height * 16
    d = pkg.hip.rtu_device_alloc(ctx._h, nbytes)
    assert d
    ms = ctx.time_render(fr, d, None, 3)
    assert 0 < ms < 1000
    out = np.empty((g.height, g.width, 4), np.float32)
    assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, nbytes) == 0
    ref, _ = ctx.render(fr)
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32))
    pkg.hip.rtu_device_free(ctx._h, d)


@pytest.mark.parametrize("tag", TEX_TAGS)
@pytest.mark.parametrize("size", [None, (800, 600)])
def test_textured_scene(pkg, orc, ctx, golden, tag, size):
    """SURVEY row f2 — Project7: checkerboards on a plane and a sphere, a PNG on the teapot (through its
    texture vertices), PNG background and environment maps, mirror and glass. z bit-exact; counters
    equal; RGB within the bar against the oracle (pinned bit-exact to the reference on this scene)."""
    g = golden(tag)
    scene = g.scene(pkg)
    W, H = size or (g.width, g.height)
    gpu, gstats = render_gpu(pkg, ctx, scene, W, H)
    fast, _ = render_gpu(pkg, ctx, scene, W, H, stats=False)
    assert np.array_equal(gpu.view(np.uint32), fast.view(np.uint32)), "fast and counting variants differ"
    cpu, cstats = orc.render(scene, W, H, threads=8)
    check_against(gpu, cpu, orc)
    assert gstats == cstats
    if size is None:
        assert sha256(gpu[..., 3]) == g.meta["sha256_z_f32"]


@pytest.mark.parametrize("coop", [True, False])
def test_textured_synthetic_scene(pkg, orc, ctx, tmp_path, coop):
    """Textures on every TexturedColor of a material (diffuse, specular, reflection, refraction), with
    rotated / scaled / translated TextureMaps, a PPM file texture on a mesh through its texture
    vertices, a checker background under a transform and a file environment map seen through glass
    and by mirror rays. GPU against the oracle (whose texture code is pinned to the reference)."""
    import math, random
    rnd = random.Random(11)
    Wt, Ht = 33, 17
    (tmp_path / "noise.ppm").write_bytes(b"P6\n%d %d\n255\n" % (Wt, Ht) + bytes(rnd.randrange(256) for _ in range(Wt * Ht * 3)))
    # a bumpy disc with texture vertices
    verts, tverts, faces = [(0.0, 0.0, 0.3)], [(0.5, 0.5, 0.0)], []
    n = 48
    for i in range(n):
        a = 2 * math.pi * i / n
        verts.append((3 * math.cos(a), 3 * math.sin(a), 0.2 * math.sin(5 * a)))
        tverts.append((0.5 + 0.5 * math.cos(a), 0.5 + 0.5 * math.sin(a), 0.0))
    for i in range(n):
        faces.append((1, 2 + i, 2 + (i + 1) % n))
    with open(tmp_path / "disc.obj", "w") as f:
        for v in verts: f.write("v %r %r %r\n" % v)
        for t in tverts: f.write("vt %r %r %r\n" % t)
        f.write("vn 0 0 1\n")
        for (i, j, k) in faces: f.write("f %d/%d/1 %d/%d/1 %d/%d/1\n" % (i, i, j, j, k, k))
    xml = tmp_path / "tex.xml"
    xml.write_text("""<xml><scene>
      <background r="0.9" g="0.8" b="1" texture="checkerboard"><color1 r="0.1" g="0.2" b="0.3"/><color2 r="0.9" g="0.9" b="0.7"/>
        <scale x="0.2" y="0.1"/><rotate angle="20" z="1"/></background>
      <environment value="0.8" texture="{d}/noise.ppm"><scale value="0.5"/></environment>
      <object type="plane" name="floor" material="floor"><scale value="30"/><translate z="-2"/></object>
      <object type="obj" name="{d}/disc.obj" material="disc"><rotate angle="25" x="1"/><translate x="-2" y="1" z="0.5"/></object>
      <object type="sphere" name="glass" material="glass"><scale value="1.6"/><translate x="2.5" y="-1" z="0.4"/></object>
      <object type="sphere" name="ball" material="ball"><scale value="1.2"/><translate x="0" y="3" z="0"/></object>
      <material type="blinn" name="floor"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.2" g="0.2" b="0.2"/><color2 r="0.8" g="0.7" b="0.6"/>
          <scale value="0.05"/><rotate angle="30" z="1"/></diffuse><specular value="0.2"/><glossiness value="20"/>
        <reflection value="0.5" texture="checkerboard"><color1 r="0" g="0" b="0"/><color2 r="1" g="1" b="1"/><scale value="0.25"/></reflection></material>
      <material type="blinn" name="disc"><diffuse texture="{d}/noise.ppm"><translate x="0.25" y="0.1"/></diffuse>
        <specular r="1" g="1" b="1" texture="{d}/noise.ppm"><scale value="3"/></specular><glossiness value="35"/></material>
      <material type="blinn" name="glass"><diffuse value="0.05"/><specular value="0.9"/><glossiness value="90"/>
        <refraction index="1.45" value="0.9" texture="checkerboard"><color1 r="0.6" g="0.9" b="0.6"/><color2 r="1" g="1" b="1"/><scale x="0.1" y="0.2"/></refraction></material>
      <material type="blinn" name="ball"><diffuse r="0.9" g="0.9" b="0.9" texture="{d}/noise.ppm"><scale x="0.5" y="1"/><rotate angle="45" z="1"/></diffuse>
        <specular value="0.5"/><glossiness value="50"/><reflection value="0.3"/></material>
      <light type="ambient" name="a"><intensity value="0.2"/></light>
      <light type="direct" name="d"><intensity value="0.6"/><direction x="-0.4" y="0.5" z="-1"/></light>
      <light type="point" name="p"><intensity value="0.5"/><position x="6" y="-8" z="9"/></light>
    </scene><camera><position x="1" y="-13" z="5"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="45"/>
      <width value="240"/><height value="160"/></camera></xml>""".format(d=tmp_path))
    scene = pkg.Scene.from_xml(str(xml))
    assert scene.desc.n_textures == 5  # four checkerboards + the PPM (one texture, shared by name)
    W, H = 240, 160
    ctx.upload(scene)
    fr = pkg.frame_setup(scene.desc.camera, W, H)
    fr.coop_threshold = 10 ** 9 if coop else 1
    fast, _ = ctx.render(fr)
    cnt, gst = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
    cpu, cst = orc.render(scene, W, H, threads=4)
    assert np.array_equal(fast.view(np.uint32), cnt.view(np.uint32)), "fast and counting variants differ"
    check_against(fast, cpu, orc)
    assert gst == cst
    assert gst["secondary_rays"] > 5000 and gst["mesh_entries"] > 2000
    assert len(np.unique((np.clip(fast[..., :3], 0, 1) * 255).astype(np.uint8).reshape(-1, 3), axis=0)) > 2000  # textures visible


def test_full_size_properties(pkg, ctx, golden):
    """Size-independent properties at the BASELINE resolution: misses carry BIGFLOAT and
    the background colour, hits have 0 < z < BIGFLOAT, re-rendering is idempotent."""
    g = golden("teapot2_1080")
    scene = g.scene(pkg)
    a, st = render_gpu(pkg, ctx, scene, g.width, g.height)
    b, _ = render_gpu(pkg, ctx, scene, g.width, g.height)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    miss = a[..., 3] == np.float32(1e30)
    assert int((~miss).sum()) == st["primary_hits"]
    assert np.all(a[miss][:, :3] == 0)  # NULL-map background samples black
    assert np.all(a[~miss][:, 3] > 0)
    assert np.all(np.isfinite(a[..., :3]))


def test_begin_render_dropin(pkg, orc, golden, tmp_path):
    """BeginRender()-style asynchronous entry of the host library writes Result.png and
    ZBuffer.png equal to the reference's decoded pixels (z exact, RGB +-1)."""
    from conftest import read_png
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    img = pkg.Image(g.width, g.height)
    devs = (ctypes.c_int * 1)(0)
    rp, zp = str(tmp_path / "Result.png"), str(tmp_path / "ZBuffer.png")
    job = pkg.host.rtu_begin_render(scene._h, img._h, devs, 1, rp.encode(), zp.encode())
    assert job
    assert pkg.host.rtu_render_wait(job) == 0, pkg.host.rtu_host_last_error()
    pkg.host.rtu_render_job_free(job)
    assert pkg.host.rtu_image_is_done(img._h)
    zimg = read_png(zp)
    assert np.array_equal(zimg, g.npz["zbuffer_u8"])
    rgb = read_png(rp)
    assert np.abs(rgb.astype(np.int32) - g.npz["result_u8"].astype(np.int32)).max() <= RGB8_TOL


@pytest.mark.parametrize("tag,n_ctx", [("teapot2_240x135", 3), ("p4_240x135", 2), ("teapot2_1080", 3), ("p13_200x150", 5)])
def test_begin_render_on_several_contexts(pkg, golden, tag, n_ctx, tmp_path):
    """The N-device code of the C++ drop-in (host/begin_render.cpp: main.cpp:29-64's SpawnRenderThreads over GPUs) on the one-GPU
    box: device_ids = {0, 0, ...} makes N contexts on GPU 0, each rendering its interleaved 8-row bands on its own stream,
    collected by asynchronous copies that are all in flight together (RCCL needs N distinct GPUs: with duplicates the job takes
    the copy path and says so). The PNGs must be the reference's: ZBuffer.png exact, Result.png within one level."""
    from conftest import read_png
    g = golden(tag)
    scene = g.scene(pkg)
    img = pkg.Image(g.width, g.height)
    devs = (ctypes.c_int * n_ctx)(*([0] * n_ctx))
    rp, zp = str(tmp_path / "Result.png"), str(tmp_path / "ZBuffer.png")
    job = pkg.host.rtu_begin_render(scene._h, img._h, devs, n_ctx, rp.encode(), zp.encode())
    assert job
    assert pkg.host.rtu_render_wait(job) == 0, pkg.host.rtu_host_last_error()
    assert pkg.host.rtu_render_gather_kind(job) == 2
    pkg.host.rtu_render_job_free(job)
    assert pkg.host.rtu_image_is_done(img._h)
    assert np.array_equal(read_png(zp), read_png(os.path.join(g.dir, "ZBuffer.png")))
    ref = read_png(os.path.join(g.dir, "Result.png"))
    assert np.abs(read_png(rp).astype(np.int32) - ref.astype(np.int32)).max() <= RGB8_TOL


def test_begin_render_rccl_path_loads_and_runs(pkg, golden, tmp_path, monkeypatch):
    """The RCCL branch of the drop-in needs as many distinct GPUs as contexts; on the one-GPU box RTU_FORCE_RCCL sends a single
    context through it: librccl.so is found and its entry points resolved at run time, a communicator is created on the GPU,
    the (empty) send / receive group is issued on the context's stream, the frame arrives through the same copies."""
    from conftest import read_png
    monkeypatch.setenv("RTU_FORCE_RCCL", "1")
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    img = pkg.Image(g.width, g.height)
    devs = (ctypes.c_int * 1)(0)
    rp, zp = str(tmp_path / "Result.png"), str(tmp_path / "ZBuffer.png")
    job = pkg.host.rtu_begin_render(scene._h, img._h, devs, 1, rp.encode(), zp.encode())
    assert job
    assert pkg.host.rtu_render_wait(job) == 0, pkg.host.rtu_host_last_error()
    assert pkg.host.rtu_render_gather_kind(job) == 3, "the RCCL path was not taken"
    pkg.host.rtu_render_job_free(job)
    assert np.array_equal(read_png(zp), g.npz["zbuffer_u8"])


def test_exact_ties_follow_the_reference_order(pkg, orc, ctx, tmp_path):
    """Two coincident triangles give bitwise-equal t; the reference keeps whichever its BVH
    walk tests first (strict `t < hInfo.z`). The fast path walks a different (SAH) tree, must
    notice the tie and redo the ray in the reference's order: duplicated geometry with
    DIFFERENT vertex normals makes a wrong winner visible in the colour."""
    import random
    rnd = random.Random(7)
    verts, norms, faces = [], [], []
    def add_tri(a, b, c, n):
        base = len(verts)
        verts.extend([a, b, c])
        norms.extend([n, n, n])
        faces.append((base + 1, base + 2, base + 3))
    for i in range(40):  # 40 triangles, each present twice with different shading normals
        cx, cy = rnd.uniform(-4, 4), rnd.uniform(-4, 4)
        a, b, c = (cx, cy, 0.1 * i), (cx + 1.5, cy, 0.1 * i), (cx, cy + 1.5, 0.1 * i)
        add_tri(a, b, c, (0, 0, 1))
        add_tri(a, b, c, (0.6, 0, 0.8))
    obj = tmp_path / "dup.obj"
    with open(obj, "w") as f:
        for v in verts: f.write("v %r %r %r\n" % v)
        for n in norms: f.write("vn %r %r %r\n" % n)
        for (i, j, k) in faces: f.write("f %d//%d %d//%d %d//%d\n" % (i, i, j, j, k, k))
    xml = tmp_path / "dup.xml"
    xml.write_text("""<xml><scene>
      <object type="obj" name="%s" material="m"/>
      <material type="blinn" name="m"><diffuse r="0.8" g="0.5" b="0.2"/><specular value="0.5"/></material>
      <light type="direct" name="d"><intensity value="1"/><direction x="-0.3" y="0.2" z="-1"/></light>
      <light type="ambient" name="a"><intensity value="0.1"/></light>
    </scene><camera><position x="0" y="0" z="20"/><target x="0" y="0" z="0"/><up x="0" y="1" z="0"/><fov value="40"/>
      <width value="160"/><height value="120"/></camera></xml>""" % obj)
    scene = pkg.Scene.from_xml(str(xml))
    W, H = 160, 120
    fast, _ = render_gpu(pkg, ctx, scene, W, H, stats=False)
    cnt, gst = render_gpu(pkg, ctx, scene, W, H, stats=True)
    cpu, cst = orc.render(scene, W, H, threads=2)
    assert np.array_equal(fast.view(np.uint32), cnt.view(np.uint32)), "tie resolved differently from the reference order"
    check_against(fast, cpu, orc)
    assert gst == cst
    assert gst["primary_hits"] > 1000


def test_degenerate_mesh_deep_trees(pkg, orc, ctx, tmp_path):
    """300 triangles in geometric progression: the reference's mean-split BVH is 42 levels deep (its
    walk needs most of the 48 stack entries); the SAH tree stays shallow. Must be the reference's image."""
    verts, faces = [], []
    x = 1e-3
    for i in range(300):
        sz = x * 0.4
        y = ((i * 37) % 11 - 5) * sz * 0.3
        base = len(verts)
        verts += [(x, y, 0.0), (x + sz, y, 0.01 * sz), (x, y + sz, 0.0)]
        faces.append((base + 1, base + 2, base + 3))
        x *= 1.05
    obj = tmp_path / "geo.obj"
    with open(obj, "w") as f:
        for v in verts: f.write("v %r %r %r\n" % v)
        f.write("vn 0 0 1\n")
        for (i, j, k) in faces: f.write("f %d//1 %d//1 %d//1\n" % (i, j, k))
    xml = tmp_path / "geo.xml"
    xml.write_text("""<xml><scene>
      <object type="obj" name="%s" material="m"/>
      <material type="blinn" name="m"><diffuse r="0.8" g="0.5" b="0.2"/><specular value="0.5"/><reflection value="0.3"/></material>
      <light type="direct" name="d"><intensity value="1"/><direction x="-0.3" y="0.2" z="-1"/></light>
      <light type="ambient" name="a"><intensity value="0.1"/></light>
    </scene><camera><position x="%r" y="0" z="%r"/><target x="%r" y="0" z="0"/><up x="0" y="1" z="0"/><fov value="50"/>
      <width value="160"/><height value="120"/></camera></xml>""" % (obj, x * 0.3, x * 0.5, x * 0.3))
    scene = pkg.Scene.from_xml(str(xml))
    W, H = 160, 120
    fast, _ = render_gpu(pkg, ctx, scene, W, H, stats=False)
    info = ctx.mesh_info(0)
    assert info["faces"] == 300 and info["sah_depth"] <= 32, info
    cnt, gst = render_gpu(pkg, ctx, scene, W, H, stats=True)
    cpu, cst = orc.render(scene, W, H, threads=2)
    assert np.array_equal(fast.view(np.uint32), cnt.view(np.uint32))
    check_against(fast, cpu, orc)
    assert gst == cst
    assert gst["primary_hits"] > 500


def _write_uv_mesh(path, nu, nv, fn):
    """OBJ of a parametric surface fn(u, v) -> (x, y, z), smooth normals by finite differences."""
    import math
    verts, norms, faces = [], [], []
    for i in range(nu + 1):
        for j in range(nv + 1):
            u, v = i / nu, j / nv
            p = fn(u, v)
            du = [a - b for a, b in zip(fn(u + 1e-4, v), fn(u - 1e-4, v))]
            dv = [a - b for a, b in zip(fn(u, v + 1e-4), fn(u, v - 1e-4))]
            n = (du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0])
            ln = math.sqrt(sum(c * c for c in n)) or 1.0
            verts.append(p)
            norms.append(tuple(c / ln for c in n))
    for i in range(nu):
        for j in range(nv):
            a = i * (nv + 1) + j + 1
            b, c, d = a + 1, a + nv + 1, a + nv + 2
            faces += [(a, c, b), (b, c, d)]
    with open(path, "w") as f:
        for v in verts: f.write("v %r %r %r\n" % tuple(v))
        for n in norms: f.write("vn %r %r %r\n" % n)
        for (i, j, k) in faces: f.write("f %d//%d %d//%d %d//%d\n" % (i, i, j, j, k, k))
    return len(faces)


@pytest.mark.parametrize("coop", [True, False])
def test_two_meshes_nested_transforms_glass_and_mirror(pkg, orc, ctx, tmp_path, coop):
    """A scene none of the reference's files has: two DIFFERENT meshes (one instanced twice) under
    three levels of rotated / non-uniformly scaled groups, a glass sphere in front of them, a
    mirror floor, a point and a direct light. GPU (both kernel variants, cooperative or wide stage 2)
    against the CPU oracle: z bit-exact, RGB within the bar, all counters equal."""
    import math
    def torus(u, v):
        a, b = 2 * math.pi * u, 2 * math.pi * v
        return ((2 + 0.7 * math.cos(b)) * math.cos(a), (2 + 0.7 * math.cos(b)) * math.sin(a), 0.7 * math.sin(b))
    def blob(u, v):
        a, b = 2 * math.pi * u, math.pi * (v - 0.5)
        r = 1.5 + 0.3 * math.sin(5 * a) * math.cos(3 * b)
        return (r * math.cos(b) * math.cos(a), r * math.cos(b) * math.sin(a), r * math.sin(b))
    n1 = _write_uv_mesh(tmp_path / "torus.obj", 40, 16, torus)
    n2 = _write_uv_mesh(tmp_path / "blob.obj", 36, 18, blob)
    assert n1 == 1280 and n2 == 1296
    xml = tmp_path / "two.xml"
    xml.write_text("""<xml><scene>
      <object type="plane" name="floor" material="mirror"><scale value="40"/><translate z="-4"/></object>
      <object name="g1"><rotate angle="20" z="1"/><translate x="1" y="2" z="0"/>
        <object type="obj" name="{d}/torus.obj" material="red"><scale x="1.2" y="0.8" z="1.5"/><rotate angle="35" x="1"/></object>
        <object name="g2"><scale value="0.7"/><rotate angle="-40" y="1"/><translate x="-5" y="1" z="1"/>
          <object type="obj" name="{d}/blob.obj" material="green"><rotate angle="15" x="1"/></object>
          <object name="g3"><translate x="0" y="-5" z="2"/><rotate angle="70" z="1"/>
            <object type="obj" name="{d}/torus.obj" material="glossy"><scale value="0.6"/></object>
            <object type="sphere" name="s_in" material="green"><scale value="0.5"/><translate z="2"/></object>
          </object>
        </object>
      </object>
      <object type="sphere" name="glass" material="glass"><scale x="2.2" y="2.2" z="2.6"/><translate x="2" y="-7" z="1"/></object>
      <material type="blinn" name="red"><diffuse r="0.8" g="0.2" b="0.2"/><specular value="0.6"/><glossiness value="40"/></material>
      <material type="blinn" name="green"><diffuse r="0.2" g="0.7" b="0.3"/><specular value="0.3"/><glossiness value="10"/></material>
      <material type="blinn" name="glossy"><diffuse r="0.5" g="0.5" b="0.6"/><specular value="0.8"/><glossiness value="80"/><reflection value="0.4"/></material>
      <material type="blinn" name="mirror"><diffuse r="0.2" g="0.2" b="0.2"/><specular value="0.7"/><glossiness value="30"/><reflection value="0.6"/></material>
      <material type="blinn" name="glass"><diffuse r="0.05" g="0.05" b="0.05"/><specular value="0.9"/><glossiness value="100"/>
        <refraction index="1.5" value="0.9"/><absorption r="0.02" g="0.01" b="0.03"/></material>
      <light type="ambient" name="a"><intensity value="0.15"/></light>
      <light type="direct" name="d"><intensity value="0.5"/><direction x="0.4" y="0.6" z="-1"/></light>
      <light type="point" name="p"><intensity value="0.6"/><position x="-6" y="-12" z="14"/></light>
    </scene><camera><position x="3" y="-24" z="9"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="38"/>
      <width value="256"/><height value="160"/></camera></xml>""".format(d=tmp_path))
    scene = pkg.Scene.from_xml(str(xml))
    assert scene.desc.n_meshes == 2
    W, H = 256, 160
    ctx.upload(scene)
    fr = pkg.frame_setup(scene.desc.camera, W, H)
    fr.coop_threshold = 10 ** 9 if coop else 1
    fast, _ = ctx.render(fr)
    frs = pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True)
    cnt, gst = ctx.render(frs, stats=True)
    cpu, cst = orc.render(scene, W, H, threads=4)
    assert np.array_equal(fast.view(np.uint32), cnt.view(np.uint32)), "fast and counting variants differ"
    check_against(fast, cpu, orc)
    assert gst == cst
    assert gst["secondary_rays"] > 5000 and gst["mesh_entries"] > 10000


def test_frame_capacity_overflow_is_detected_and_repaired(pkg, orc, tmp_path):
    """Level >= 1 frame arrays are provisioned for one frame per pixel; a view filled by a glass +
    mirror sphere inside a room spawns up to three child frames per pixel. The synchronous entry
    must notice the overflow, double the capacity and render again (transparently); the
    asynchronous one must report RTU_ERR_CAPACITY from rtu_frame_status and succeed on the retry."""
    xml = tmp_path / "glassroom.xml"
    xml.write_text("""<xml><scene>
      <object type="sphere" name="room" material="wall"><scale value="60"/></object>
      <object type="sphere" name="ball" material="glassmirror"><scale value="9"/><translate x="0" y="0" z="0"/></object>
      <material type="blinn" name="wall"><diffuse r="0.7" g="0.6" b="0.5"/><specular value="0.2"/><glossiness value="10"/></material>
      <material type="blinn" name="glassmirror"><diffuse r="0.1" g="0.1" b="0.1"/><specular value="0.8"/><glossiness value="60"/>
        <reflection value="0.4"/><refraction index="1.4" value="0.7"/></material>
      <light type="ambient" name="a"><intensity value="0.3"/></light>
      <light type="point" name="p"><intensity value="0.8"/><position x="10" y="-20" z="25"/></light>
    </scene><camera><position x="0" y="-14" z="0"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="70"/>
      <width value="128"/><height value="96"/></camera></xml>""")
    scene = pkg.Scene.from_xml(str(xml))
    W, H = 128, 96
    cpu, cst = orc.render(scene, W, H, threads=4)
    ctx = pkg.Context(0)   # a fresh context: capacity scale 1
    try:
        ctx.upload(scene)
        fr = pkg.frame_setup(scene.desc.camera, W, H)
        nbytes = W * H * 16
        d = pkg.hip.rtu_device_alloc(ctx._h, nbytes)
        ctx.render_device(fr, d, None)
        # the report is sticky: a later launch sequence that fits (the camera turned away from the ball: bare wall, no
        # child frames) queued behind the overflowed one must not erase it
        cam_away = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        for k in range(3):
            cam_away.dir[k] = -cam_away.dir[k]
        d2 = pkg.hip.rtu_device_alloc(ctx._h, nbytes)
        ctx.render_device(pkg.frame_setup(cam_away, W, H), d2, None)
        with pytest.raises(pkg.RtuError) as e:
            ctx.frame_status()
        assert e.value.code == pkg.RTU_ERR_CAPACITY
        ctx.frame_status()  # ... and is cleared by being read
        away = np.empty((H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, away.ctypes.data, d2, nbytes) == 0
        pkg.hip.rtu_device_free(ctx._h, d2)
        assert (away[..., 3] > 40).all()  # only the room's wall in view
        for _ in range(8):  # every report grows the capacity of at least one more recursion level
            ctx.render_device(fr, d, None)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as err:
                assert err.code == pkg.RTU_ERR_CAPACITY
        else:
            raise AssertionError("capacity never sufficed")
        out = np.empty((H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, nbytes) == 0
        pkg.hip.rtu_device_free(ctx._h, d)
        check_against(out, cpu, orc)
        frames, _ = ctx.frame_counts()
        # more child frames than pixels in some level: the case the test is about (the wall seen through and in the ball is
        # childless — settled without a frame since round 3 —, the ball's own inside keeps multiplying)
        assert max(frames[1:]) > W * H, frames
    finally:
        ctx.close()
    ctx2 = pkg.Context(0)  # synchronous entry on a fresh context: transparent retry
    try:
        ctx2.upload(scene)
        img, gst = ctx2.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
        check_against(img, cpu, orc)
        assert gst == cst
    finally:
        ctx2.close()


@pytest.mark.parametrize("tag", ["p4_240x135", "teapot2_240x135", "p13_200x150", "p7_200x150"])
@pytest.mark.parametrize("level", [1, 2, 3, 4, 5])
def test_tail_kernel_any_cut_level(pkg, ctx, golden, tag, level):
    """Recursion levels >= `level` evaluated by k_tail (one wavefront per frame of that level, its
    whole Shade() subtree inside the wavefront) instead of the per-level kernels: the same image bit
    for bit whatever the cut level and however many frames it holds (p4: tens of thousands)."""
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    fr = pkg.frame_setup(scene.desc.camera, g.width, g.height)
    assert pkg.hip.rtu_debug_tail_from(ctx._h, 6) == 0
    ref, _ = ctx.render(fr)
    assert pkg.hip.rtu_debug_tail_from(ctx._h, level) == 0
    tail, _ = ctx.render(fr)
    assert np.array_equal(ref.view(np.uint32), tail.view(np.uint32))


@pytest.mark.parametrize("tag,coop", [("teapot2_240x135", True), ("teapot2_240x135", False), ("p11_240x135", False)])
def test_walk_stack_overflow_falls_back_to_the_reference_tree(pkg, ctx, golden, tag, coop):
    """A walk of the 4-wide / 8-wide tree that would need more stack than it has finishes on the
    reference's tree (like an exact tie). Forced here by a test hook that leaves the walks 3
    entries: the frame must not change in any bit, on the cooperative and the wide kernels."""
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    fr = pkg.frame_setup(scene.desc.camera, g.width, g.height)
    fr.coop_threshold = 10 ** 9 if coop else 1
    ref, _ = ctx.render(fr)
    assert pkg.hip.rtu_debug_walk_stack_limit(ctx._h, 3) == 0
    small, _ = ctx.render(fr)
    assert np.array_equal(ref.view(np.uint32), small.view(np.uint32))
    ctx.upload(scene)  # restores the limit


def test_exact_division(pkg, ctx):
    """(float)((double)n * (1.0/(double)d)) == n / d bit for bit (rtu_intersect.h fdiv): 2^31
    pseudo-random operand pairs incl. subnormals, zeros, infinities, NaNs, near-1 quotients."""
    bad = ctypes.c_ulonglong(123)
    for seed in (0, 0x1234567):
        assert pkg.hip.rtu_selftest_division(ctx._h, 1 << 30, seed, ctypes.byref(bad)) == 0
        assert bad.value == 0, "%d quotients differ" % bad.value


def test_reordered_primitive_tests_equal_the_literal_order(pkg, ctx):
    """Sphere / plane: bounding-box test skipped when implied vs the reference's order, 2^28 rays."""
    for seed in (1, 2026):
        bad = ctypes.c_ulonglong(123)
        assert pkg.hip.rtu_selftest_primitives(ctx._h, 1 << 28, seed, ctypes.byref(bad)) == 0
        assert bad.value == 0


def test_errors_are_codes_not_crashes(pkg, ctx, golden):
    g = golden("p1_256")
    scene = g.scene(pkg)
    fr = pkg.frame_setup(scene.desc.camera, 16, 16)
    fresh = pkg.Context(0)
    out = np.empty((16, 16, 4), np.float32)
    assert pkg.hip.rtu_render_frame(fresh._h, ctypes.byref(fr), out.ctypes.data, None) == pkg.RTU_ERR_NO_SCENE
    fresh.close()
    bad = pkg.frame_setup(scene.desc.camera, 16, 16, shard_rank=2, shard_count=2)
    ctx.upload(scene)
    assert pkg.hip.rtu_render_frame(ctx._h, ctypes.byref(bad), out.ctypes.data, None) == pkg.RTU_ERR_ARG
    err = ctypes.c_int(0)
    assert not pkg.hip.rtu_create_context(9999, ctypes.byref(err))
    assert err.value == pkg.RTU_ERR_NO_DEVICE


@pytest.mark.parametrize("tag,shards", [("teapot2_240x135", 1), ("p4_240x135", 1), ("p7_200x150", 1), ("p11_240x135", 3)])
def test_frames_in_flight_equal_single_frames(pkg, ctx, golden, tag, shards):
    """rtu_render_frames_device: a batch of frames with different cameras rendered by one launch sequence —
    every image equals the one rtu_render_frame gives for that frame alone, bit for bit (fast and counting
    variants; sharded; textured), and a frame with the golden's camera still has the golden's z."""
    import copy
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    n = 5
    for rank in range(shards):
        frames = []
        for i in range(n):
            cam = copy.copy(scene.desc.camera)
            cam = type(cam).from_buffer_copy(bytes(cam))
            cam.pos[0] += 0.37 * i
            cam.pos[2] += 0.11 * i * i
            cam.fov += 1.5 * i
            frames.append(pkg.frame_setup(cam, W, H, shard_rank=rank, shard_count=shards))
        rows = pkg.shard_rows(frames[0])
        singles = [ctx.render(f)[0] for f in frames]
        assert not np.array_equal(singles[0], singles[1])
        d = pkg.hip.rtu_device_alloc(ctx._h, n * rows * W * 16)
        for stats in (False, True):
            for f in frames:
                f.collect_stats = 1 if stats else 0
            ctx.render_frames_device(frames, d)
            ctx.frame_status()
            got = np.empty((n, rows, W, 4), np.float32)
            assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
            for i in range(n):
                assert np.array_equal(got[i].view(np.uint32), singles[i].view(np.uint32)), "frame %d of the batch differs (stats=%s)" % (i, stats)
        if shards == 1:
            assert sha256(got[0][..., 3]) == g.meta["sha256_z_f32"]
        # any tail cut level gives the same images
        for f in frames:
            f.collect_stats = 0
        for level in (1, 3):
            assert pkg.hip.rtu_debug_tail_from(ctx._h, level) == 0
            ctx.render_frames_device(frames, d)
            ctx.frame_status()
            assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
            assert all(np.array_equal(got[i].view(np.uint32), singles[i].view(np.uint32)) for i in range(n))
        pkg.hip.rtu_device_free(ctx._h, d)
    # errors: frames that differ in more than their cameras, too many frames, sampled frames
    a, b = pkg.frame_setup(scene.desc.camera, W, H), pkg.frame_setup(scene.desc.camera, W, H + 8)
    d = pkg.hip.rtu_device_alloc(ctx._h, 128 * (H + 8) * W * 16)
    arr = (pkg.RtuFrameDesc * 2)(a, b)
    assert pkg.hip.rtu_render_frames_device(ctx._h, arr, 2, d, None) == pkg.RTU_ERR_ARG
    arr129 = (pkg.RtuFrameDesc * 129)(*([a] * 129))  # RTU_MAX_FRAMES_IN_FLIGHT is 128
    assert pkg.hip.rtu_render_frames_device(ctx._h, arr129, 129, d, None) == pkg.RTU_ERR_ARG
    arr128 = (pkg.RtuFrameDesc * 128)(*([a] * 128))
    assert pkg.hip.rtu_render_frames_device(ctx._h, arr128, 128, d, None) == 0
    ctx.frame_status()
    last = np.empty((H, W, 4), np.float32)
    assert pkg.hip.rtu_copy_to_host(ctx._h, last.ctypes.data, d + 127 * H * W * 16, last.nbytes) == 0
    assert sha256(last[..., 3]) == g.meta["sha256_z_f32"] or shards != 1  # the 128th frame of the batch is the golden frame too
    s = pkg.frame_setup(scene.desc.camera, W, H, samples=2)
    arr = (pkg.RtuFrameDesc * 2)(s, s)
    assert pkg.hip.rtu_render_frames_device(ctx._h, arr, 2, d, None) == pkg.RTU_ERR_ARG
    pkg.hip.rtu_device_free(ctx._h, d)


def test_pack_image_matches_the_host_postprocess(pkg, orc, ctx, golden):
    """rtu_pack_image_device (what a multi-GPU gather moves: float z + Color24) against the host post-process:
    z identical, every 8-bit channel within one level (binary64 pow on both sides: equal in practice)."""
    for tag in ("teapot2_240x135", "p4_240x135", "p7_200x150"):
        g = golden(tag)
        scene = g.scene(pkg)
        ctx.upload(scene)
        W, H = g.width, g.height
        fr = pkg.frame_setup(scene.desc.camera, W, H)
        n = W * H
        d = pkg.hip.rtu_device_alloc(ctx._h, n * 16)
        dz = pkg.hip.rtu_device_alloc(ctx._h, n * 4)
        drgb = pkg.hip.rtu_device_alloc(ctx._h, n * 3)
        ctx.render_device(fr, d)
        ctx.pack_image_device(d, n, dz, drgb)
        ctx.frame_status()
        img = np.empty((H, W, 4), np.float32)
        z = np.empty((H, W), np.float32)
        rgb = np.empty((H, W, 3), np.uint8)
        assert pkg.hip.rtu_copy_to_host(ctx._h, img.ctypes.data, d, n * 16) == 0
        assert pkg.hip.rtu_copy_to_host(ctx._h, z.ctypes.data, dz, n * 4) == 0
        assert pkg.hip.rtu_copy_to_host(ctx._h, rgb.ctypes.data, drgb, n * 3) == 0
        want8, _, _ = orc.postprocess(img)
        assert np.array_equal(z.view(np.uint32), img[..., 3].view(np.uint32))
        dd = np.abs(rgb.astype(np.int32) - want8.astype(np.int32))
        assert dd.max() <= RGB8_TOL
        print("%s: %d of %d channel values differ from the host's" % (tag, int((dd > 0).sum()), n * 3))
        assert sha256(z) == g.meta["sha256_z_f32"]
        for p_ in (d, dz, drgb):
            pkg.hip.rtu_device_free(ctx._h, p_)


@pytest.mark.parametrize("tag,fif", [("teapot2_240x135", 1), ("p11_240x135", 1), ("p4_240x135", 1), ("p7_200x150", 1), ("teapot2_240x135", 4),
                                     ("p13_200x150", 3)])
def test_touched_bytes_mode_is_the_fast_variant_counting_itself(pkg, ctx, golden, tag, fif):
    """collect_stats == 2 (what bench.py's roofline is computed from): the kernels of the FAST variant — same trees, same
    culling, same two stages — with per-kernel counters of what they touch. Its images are the fast variant's bit for bit, its
    ray bookkeeping adds up (every pixel starts one walk in k_primary; stage 2 restarts exactly the deferred ones), and it walks
    fewer boxes than the reference-counting variant (whose counters equal the oracle's)."""
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    textured = scene.desc.n_textures > 0
    cams = []
    for i in range(fif):
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        cam.pos[0] += 0.4 * i
        cams.append(cam)
    fast = [ctx.render(pkg.frame_setup(c, W, H))[0] for c in cams]
    d = pkg.hip.rtu_device_alloc(ctx._h, fif * W * H * 16)
    frames = [pkg.frame_setup(c, W, H, collect_stats=2) for c in cams]
    for coop in (1, 10 ** 9):  # one lane per ray / eight lanes per ray in stage 2
        for f in frames:
            f.coop_threshold = coop
        if fif == 1:
            ctx.render_device(frames[0], d, None)
        else:
            ctx.render_frames_device(frames, d, None)
        ctx.frame_status()
        t = ctx.touched(textured)
        out = np.empty((fif, H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
        for i in range(fif):
            assert np.array_equal(out[i].view(np.uint32), fast[i].view(np.uint32)), "touched-bytes mode changed the image"
        _, deferred = ctx.frame_counts()
        # (a primary kernel also fires the shadow rays of the childless Shade() calls it settles itself: counted apart)
        walks = lambda k: t[k]["rays"] - t[k]["inline_shadow_rays"] if k in t else 0
        assert walks("k_primary") == fif * W * H
        st2 = walks("k_primary2") + walks("k_primary2c")
        assert st2 == deferred[0]
        assert ("k_primary2" in t) != ("k_primary2c" in t) or deferred[0] == 0
        assert t["k_primary"]["record_bytes"] >= 16 * (fif * W * H - deferred[0])  # a pixel or a frame record per finished pixel
        for name, c in t.items():
            assert c["bytes"] >= c["record_bytes"] and c["bytes"] > 0, name
            if name.startswith("k_combine"):
                assert c["rays"] == 0 and c["bytes"] == c["record_bytes"]
            if name.startswith("k_consume"):  # (the only rays it fires are the shadow rays of the childless children it settles itself)
                assert c["rays"] == c["inline_shadow_rays"]
            if name.startswith("k_trace2(") or name == "k_primary2":
                assert c["inner8"] == 0
            if name.startswith("k_trace2c") or name == "k_primary2c":
                assert c["inner4"] == 0
    pkg.hip.rtu_device_free(ctx._h, d)
    if scene.desc.n_meshes and fif == 1:
        _, ref = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
        inner = sum(c["inner4"] + c["inner8"] + c["inner_ref"] for c in t.values())
        assert 0 < inner < ref["inner_visits"]


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p4_240x135", "p11_240x135", "p13_200x150", "p7_200x150", "p5_200x150"])
def test_node_level_bounds_change_nothing_but_the_work(pkg, ctx, golden, tag):
    """a world-space box per scene node (and its screen rectangle per camera for primary rays) lets a ray skip the
    nodes it cannot touch before their transformation and exact test. Same image bit for bit with the bounds on and off
    (rtu_debug_node_bounds), single frame and frames in flight with turned cameras, both stage-2 forms — and fewer exact
    node tests with them on."""
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    cams = []
    for i in range(3):
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        cam.pos[0] += 1.3 * i
        cam.pos[2] -= 0.7 * i
        cam.fov += 9.0 * i
        cams.append(cam)
    d = pkg.hip.rtu_device_alloc(ctx._h, 3 * W * H * 16)
    res = {}
    for on in (1, 0):
        assert pkg.hip.rtu_debug_node_bounds(ctx._h, on) == 0
        imgs = []
        for coop in (1, 10 ** 9):
            fr = pkg.frame_setup(cams[0], W, H)
            fr.coop_threshold = coop
            imgs.append(ctx.render(fr)[0])
            frames = [pkg.frame_setup(c, W, H, collect_stats=2) for c in cams]
            for f in frames:
                f.coop_threshold = coop
            ctx.render_frames_device(frames, d, None)
            ctx.frame_status()
            out = np.empty((3, H, W, 4), np.float32)
            assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
            imgs.append(out)
        t = ctx.touched(scene.desc.n_textures > 0)
        res[on] = (imgs, sum(c["node_tests"] for c in t.values()), sum(c["bound_tests"] for c in t.values()))
    pkg.hip.rtu_debug_node_bounds(ctx._h, 1)
    pkg.hip.rtu_device_free(ctx._h, d)
    for a, b in zip(res[1][0], res[0][0]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "node-level bounds changed the image"
    assert res[0][2] == 0 and res[1][2] > 0
    assert res[1][1] < res[0][1], "the bounds skipped nothing: %d vs %d exact node tests" % (res[1][1], res[0][1])
    cpu, _ = __import__("__graft_entry__").load_oracle().render(scene, W, H, threads=8)
    check_against(res[1][0][0], cpu, __import__("__graft_entry__").load_oracle())


def test_node_level_bounds_on_adversarial_rays(pkg, orc, tmp_path):
    """Where the bound's argument is thinnest: a tiny sphere far from everything (its discriminant is cancellation noise:
    the bound is widened at upload), axis-parallel rays (the reference's box test ignores an axis when a direction component is
    exactly zero: odd resolution, camera on an axis, so the centre column and row have such rays), a squashed sphere as a wall,
    nested transformations. Fast variant == counting variant == oracle."""
    xml = tmp_path / "adv.xml"
    xml.write_text("""<xml><scene>
      <object type="sphere" name="wall" material="wall"><scale x="40" y="40" z="0.5"/><translate z="-3"/></object>
      <object type="sphere" name="speck" material="mirror"><scale value="0.02"/><translate x="0" y="30" z="0"/></object>
      <object name="group"><rotate angle="33" z="1"/><translate x="-2" y="4" z="0"/>
        <object type="sphere" name="ball" material="glass"><scale value="1.5"/><translate x="1" y="0" z="0.5"/>
          <object type="plane" name="card" material="wall"><scale value="0.8"/><rotate angle="90" x="1"/><translate x="0" y="-2" z="0"/></object>
        </object>
      </object>
      <object type="plane" name="floor" material="floor"><scale value="25"/><translate z="-2.5"/></object>
      <material type="blinn" name="wall"><diffuse r="0.7" g="0.6" b="0.5"/><specular value="0.2"/><glossiness value="10"/></material>
      <material type="blinn" name="floor"><diffuse r="0.4" g="0.5" b="0.4"/><specular value="0.1"/><reflection value="0.3"/></material>
      <material type="blinn" name="mirror"><diffuse value="0.1"/><specular value="0.9"/><glossiness value="90"/><reflection value="0.9"/></material>
      <material type="blinn" name="glass"><diffuse value="0.05"/><specular value="0.8"/><glossiness value="60"/><refraction index="1.45" value="0.9"/></material>
      <light type="ambient" name="a"><intensity value="0.2"/></light>
      <light type="point" name="p"><intensity value="0.7"/><position x="0" y="-5" z="20"/></light>
      <light type="direct" name="d"><intensity value="0.4"/><direction x="0" y="1" z="-1"/></light>
    </scene><camera><position x="0" y="-20" z="0"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="50"/>
      <width value="161"/><height value="101"/></camera></xml>""")
    scene = pkg.Scene.from_xml(str(xml))
    W, H = 161, 101
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        cpu, cst = orc.render(scene, W, H, threads=8)
        cnt, gst = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
        assert gst == cst
        for on in (1, 0):
            pkg.hip.rtu_debug_node_bounds(ctx._h, on)
            fast, _ = ctx.render(pkg.frame_setup(scene.desc.camera, W, H))
            assert np.array_equal(fast.view(np.uint32), cnt.view(np.uint32)), "fast (bounds %d) and counting variants differ" % on
        check_against(fast, cpu, orc)
    finally:
        ctx.close()


def test_rays_grazing_bounding_boxes_edge_on(pkg, orc, tmp_path):
    """The one way the fast tree and the reference's tree could disagree: a ray that clips a bounding box within rounding, so
    that the reference's own box arithmetic never reaches a triangle its triangle test would accept (rtu_intersect.h:
    reaches_like_the_reference). Constructed: an axis-aligned mesh (flat boxes, edges and vertices lying in box faces) under
    a transformation, seen through cameras zoomed by up to 10^7 onto a box edge, a box corner and a vertex shared by six
    triangles — every primary ray and every shadow ray of these images passes a box boundary within a few ulp. The detector
    must fire (walks finished on the reference's tree show in the touched-bytes counters) and the fast variant must equal
    the counting variant (the reference's walk) bit for bit, and the oracle."""
    obj = tmp_path / "steps.obj"
    n = 6
    verts = [(i * 0.5 - 1.5, j * 0.5 - 1.5, 0.25 * ((i + j) % 3)) for i in range(n + 1) for j in range(n + 1)]
    vid = lambda i, j: i * (n + 1) + j + 1
    faces = []
    for i in range(n):
        for j in range(n):
            faces += [(vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)), (vid(i, j), vid(i + 1, j + 1), vid(i, j + 1))]
    obj.write_text("".join("v %r %r %r\n" % v for v in verts) + "".join("f %d %d %d\n" % f for f in faces))
    sx, tx, ty, tz = 1.37, 0.11, -0.07, 0.013
    world = lambda v: (v[0] * sx + tx, v[1] * sx + ty, v[2] * sx + tz)
    targets = [world(verts[0]),                      # a corner of the mesh's bounding box
               world((-1.5, 0.25, 0.0)),             # a point of the box's x-min edge
               world(verts[vid(3, 3) - 1]),          # a vertex shared by six triangles, inside
               world((0.25, 0.25, 0.25))]            # a point of an interior edge
    W, H = 256, 48
    ctx = pkg.Context(0)
    fired = 0
    try:
        for tgt in targets:
            for fov, cam_off in ((1e-3, (0.0, 0.0, 9.0)), (3e-5, (0.4, -0.3, 7.0)), (3e-6, (0.0, 0.0, 11.0)), (1e-5, (6.0, 5.0, 0.0013))):
                xml = tmp_path / "graze.xml"
                xml.write_text("""<xml><scene><object type="obj" name="%s" material="m"><scale value="%r"/><translate x="%r" y="%r" z="%r"/></object>
                  <material type="blinn" name="m"><diffuse r="0.7" g="0.6" b="0.5"/><specular value="0.3"/></material>
                  <light type="ambient" name="a"><intensity value="0.3"/></light>
                  <light type="point" name="p"><intensity value="30"/><position x="%r" y="%r" z="%r"/></light></scene>
                  <camera><position x="%r" y="%r" z="%r"/><target x="%r" y="%r" z="%r"/><up x="0" y="1" z="0.01"/><fov value="%r"/>
                  <width value="%d"/><height value="%d"/></camera></xml>""" % (
                    obj, sx, tx, ty, tz, tgt[0] + 2.0, tgt[1] - 1.0, tgt[2] + 4.0,
                    tgt[0] + cam_off[0], tgt[1] + cam_off[1], tgt[2] + cam_off[2], tgt[0], tgt[1], tgt[2], fov, W, H))
                scene = pkg.Scene.from_xml(str(xml))
                ctx.upload(scene)
                cpu, cst = orc.render(scene, W, H, threads=8)
                cnt, gst = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
                assert gst == cst
                for coop in (1, 10 ** 9):
                    fr = pkg.frame_setup(scene.desc.camera, W, H, collect_stats=2)
                    fr.coop_threshold = coop
                    fast, _ = ctx.render(fr)
                    assert np.array_equal(fast.view(np.uint32), cnt.view(np.uint32)), "fast and counting variants differ (fov %g)" % fov
                    fired += sum(c["inner_ref"] for c in ctx.touched().values())
                check_against(fast, cpu, orc)
    finally:
        ctx.close()
    assert fired > 0, "no ray was ambiguous: the scene does not exercise the detector"


def test_tail_hint_from_another_view_is_refused_not_trusted(pkg, ctx, golden):
    """The cut level of the tail kernel is a guess from the previous launch of the same shape. Project4 seen with the camera
    turned by 30 degrees is a bare wall (no recursion at all: the guess becomes "everything below level 0 is tiny"); the next
    frame, the scene's own view, has 390 000 frames at level 1 — one wavefront per subtree would take a hundred times the
    frame. k_tail refuses such a cut level on the device; the frame is reported incomplete (RTU_ERR_CAPACITY from the
    asynchronous entry, a transparent second render from the synchronous one), rendered again level by level, and is the
    golden frame bit for bit."""
    import importlib.util, time
    spec = importlib.util.spec_from_file_location("rtu_bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    g = golden("p4_1080")
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    wall = pkg.frame_setup(bench.orbit_camera(scene.desc.camera, 30.0), W, H)
    view = pkg.frame_setup(scene.desc.camera, W, H)
    d = pkg.hip.rtu_device_alloc(ctx._h, W * H * 16)
    ctx.render_device(wall, d, None)
    ctx.frame_status()
    frames, _ = ctx.frame_counts()
    assert frames[1] == 0, frames  # the premise: nothing below level 0 in this view
    ctx.render_device(view, d, None)
    with pytest.raises(pkg.RtuError) as e:
        ctx.frame_status()
    assert e.value.code == pkg.RTU_ERR_CAPACITY
    t0 = time.perf_counter()
    ctx.render_device(view, d, None)
    ctx.frame_status()
    assert time.perf_counter() - t0 < 0.05, "the second render still went through the tail kernel"
    out = np.empty((H, W, 4), np.float32)
    assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
    pkg.hip.rtu_device_free(ctx._h, d)
    assert sha256(out[..., 3]) == g.meta["sha256_z_f32"]
    # the synchronous entry on a fresh context: wall, then the view — one call, the right frame
    c2 = pkg.Context(0)
    try:
        c2.upload(scene)
        c2.render(wall)
        img, _ = c2.render(view)
        assert np.array_equal(img.view(np.uint32), out.view(np.uint32))
    finally:
        c2.close()


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p13_200x150", "p1_256"])
def test_output_images_packed_on_the_device(pkg, ctx, golden, tag):
    """What the multi-GPU gather moves by default: the two output images, 4 bytes per pixel {Color24, z-image byte}
    (rtu_minmax_z_device -> element-wise MIN over the shards -> rtu_pack_output_device). The z-image byte must be the reference's
    ZBuffer.png bit for bit — its zmin / zmax are frame-wide, so three shards reduce their keys as the ranks' all-reduce would —
    and the colours Result.png's within one level; a batch of two frames (the second an empty view) keeps its frames apart."""
    import torch
    import importlib.util
    spec = importlib.util.spec_from_file_location("rtu_sharding", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raytracer-utah_amd", "sharding.py"))
    sharding = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(sharding)
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    away = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
    for k in range(3):
        away.dir[k] = -away.dir[k]
    for world in (1, 3, 24):  # (24 ranks > the bands of the image: some shards have no rows and must still contribute "nothing yet" keys)
        chunks, mms, bufs, rows_of = [], [], [], []
        for r in range(world):
            frs = [pkg.frame_setup(c, W, H, shard_rank=r, shard_count=world) for c in (scene.desc.camera, away)]
            rows = pkg.shard_rows(frs[0])
            buf = torch.zeros(max(2 * rows * W * 4, 4), dtype=torch.float32, device="cuda")
            if rows:
                ctx.render_frames_device(frs, buf.data_ptr(), None)
                ctx.frame_status()
            mm = torch.zeros(4, dtype=torch.int64, device="cuda")  # zeros, as bench.py allocates them: an empty shard must overwrite them
            ctx.minmax_z_device(buf.data_ptr(), rows * W, 2, mm.data_ptr(), None)
            torch.cuda.synchronize()
            bufs.append(buf); mms.append(mm); rows_of.append(rows)
        red = torch.stack(mms).min(dim=0).values  # what all_reduce(MIN) leaves on every rank
        for r in range(world):
            out = torch.zeros(max(2 * rows_of[r] * W * 4, 4), dtype=torch.uint8, device="cuda")
            ctx.pack_output_device(bufs[r].data_ptr(), rows_of[r] * W, 2, red.data_ptr(), out.data_ptr(), None)
            torch.cuda.synchronize()
            chunks.append(out.cpu().numpy())
        rgb, zimg = sharding.assemble_gathered_out4(pkg, chunks, 0, scene.desc.camera, W, H, world)
        assert np.array_equal(zimg, g.npz["zbuffer_u8"]), "z-image differs from the reference's ZBuffer.png (%d shards)" % world
        assert np.abs(rgb.astype(np.int32) - g.npz["result_u8"].astype(np.int32)).max() <= RGB8_TOL
        rgb2, zimg2 = sharding.assemble_gathered_out4(pkg, chunks, 1, scene.desc.camera, W, H, world)
        ref2, _ = ctx.render(pkg.frame_setup(away, W, H))
        import __graft_entry__ as ge
        c8, _, cz8 = ge.load_oracle().postprocess(ref2)
        assert np.array_equal(zimg2, cz8) and np.abs(rgb2.astype(np.int32) - c8.astype(np.int32)).max() <= RGB8_TOL


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p7_200x150", "mtl_160x120"])
def test_coverage_masks_with_the_camera_among_the_triangles(pkg, ctx, golden, tag):
    """The coverage masks of primary rays (k_mesh_cover: one bit per 8x8 tile and mesh — can a primary ray there touch any
    triangle?) from cameras where they are hardest: far away (the whole mesh in a few tiles), close up, INSIDE the mesh's
    bounding box and looking along its surface (triangles at and behind the camera plane: the mask must declare itself unusable),
    as frames in flight. Fast variant with the bounds and masks on == off == counting variant, bit for bit."""
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    m = ctypes.cast(scene.desc.meshes, ctypes.POINTER(pkg.RtuMesh))[0]
    base = scene.desc.camera
    cams = []
    for k, (scale, fov) in enumerate([(6.0, 20.0), (0.45, 75.0), (0.12, 100.0), (0.02, 120.0), (1.0, 170.0)]):
        cam = type(base).from_buffer_copy(base)
        # towards / past the point the camera looks at: pos + dir * distance (scenes are built around the origin)
        dist = sum(-base.pos[i] * base.dir[i] for i in range(3))
        for i in range(3):
            cam.pos[i] = base.pos[i] + base.dir[i] * dist * (1.0 - scale)
        cam.fov = fov
        cams.append(cam)
    d = pkg.hip.rtu_device_alloc(ctx._h, len(cams) * W * H * 16)
    results = {}
    for on in (1, 0):
        pkg.hip.rtu_debug_node_bounds(ctx._h, on)
        frames = [pkg.frame_setup(c, W, H) for c in cams]
        ctx.render_frames_device(frames, d, None)
        for _ in range(8):
            try:
                ctx.frame_status()
                break
            except pkg.RtuError:
                ctx.render_frames_device(frames, d, None)
        out = np.empty((len(cams), H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
        results[on] = out
    pkg.hip.rtu_debug_node_bounds(ctx._h, 1)
    pkg.hip.rtu_device_free(ctx._h, d)
    assert np.array_equal(results[1].view(np.uint32), results[0].view(np.uint32)), "bounds / coverage masks changed an image"
    for i, c in enumerate(cams):
        cnt, _ = ctx.render(pkg.frame_setup(c, W, H, collect_stats=True), stats=True)
        assert np.array_equal(cnt.view(np.uint32), results[1][i].view(np.uint32)), "camera %d: fast and counting variants differ" % i
        single, _ = ctx.render(pkg.frame_setup(c, W, H))
        assert np.array_equal(single.view(np.uint32), results[1][i].view(np.uint32))
    assert sum(bool((results[1][i][..., 3] < 1e29).any()) for i in range(len(cams))) >= 2, "the views show nothing"


def test_shadow_masks_with_lights_in_awkward_places(pkg, orc, tmp_path):
    """The shadow masks (one per non-ambient light and mesh node, made at upload: the mesh as the light sees it; a shadow ray looks
    its origin up) where they are hardest: a point light INSIDE the mesh's hull and one almost touching it (masks unusable), a point
    light far away (the mesh in a corner of its own mask), direct lights along an axis and grazing the mesh's base, six
    non-ambient lights (only the first four get masks), two mesh nodes of one mesh under different transformations. Masks and
    bounds on == off == counting variant bit for bit, counters equal to the oracle's, images within the bars of the oracle."""
    obj = tmp_path / "bumps.obj"
    n = 10
    import math
    verts = [(i * 0.4 - 2.0, j * 0.4 - 2.0, 0.6 * math.sin(0.9 * i) * math.cos(0.7 * j)) for i in range(n + 1) for j in range(n + 1)]
    vid = lambda i, j: i * (n + 1) + j + 1
    faces = []
    for i in range(n):
        for j in range(n):
            faces += [(vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)), (vid(i, j), vid(i + 1, j + 1), vid(i, j + 1))]
    obj.write_text("".join("v %r %r %r\n" % v for v in verts) + "".join("f %d %d %d\n" % f for f in faces))
    xml = tmp_path / "lights.xml"
    xml.write_text("""<xml><scene>
      <object type="obj" name="{o}" material="m"><scale value="1.2"/><translate x="-1" y="0" z="1"/></object>
      <object name="grp"><rotate angle="40" z="1"/><translate x="3.5" y="1" z="0"/>
        <object type="obj" name="{o}" material="shiny"><scale x="0.6" y="0.6" z="1.5"/><rotate angle="70" x="1"/><translate z="2"/></object></object>
      <object type="plane" name="floor" material="m"><scale value="20"/></object>
      <object type="sphere" name="ball" material="shiny"><scale value="0.8"/><translate x="0.5" y="-3" z="0.8"/></object>
      <material type="blinn" name="m"><diffuse r="0.6" g="0.6" b="0.55"/><specular value="0.3"/><glossiness value="20"/></material>
      <material type="blinn" name="shiny"><diffuse r="0.3" g="0.4" b="0.6"/><specular value="0.7"/><glossiness value="50"/><reflection value="0.4"/></material>
      <light type="ambient" name="a"><intensity value="0.1"/></light>
      <light type="point" name="inside"><intensity value="0.4"/><position x="-1" y="0" z="1.05"/></light>
      <light type="direct" name="down"><intensity value="0.3"/><direction x="0" y="0" z="-1"/></light>
      <light type="point" name="far"><intensity value="0.5"/><position x="40" y="-60" z="50"/></light>
      <light type="direct" name="grazing"><intensity value="0.3"/><direction x="1" y="0.2" z="-0.02"/></light>
      <light type="point" name="touching"><intensity value="0.2"/><position x="-1.0" y="0.4" z="1.73"/></light>
      <light type="direct" name="sixth"><intensity value="0.2"/><direction x="-0.3" y="0.5" z="-1"/></light>
    </scene><camera><position x="2" y="-11" z="6"/><target x="0.5" y="0" z="1"/><up x="0" y="0" z="1"/><fov value="45"/>
      <width value="200"/><height value="150"/></camera></xml>""".format(o=obj))
    scene = pkg.Scene.from_xml(str(xml))
    assert scene.desc.n_meshes == 1 and scene.desc.n_lights == 7
    W, H = 200, 150
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        cpu, cst = orc.render(scene, W, H, threads=8)
        cnt, gst = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
        assert gst == cst
        imgs = {}
        for on in (1, 0):
            pkg.hip.rtu_debug_node_bounds(ctx._h, on)
            for coop in (1, 10 ** 9):
                fr = pkg.frame_setup(scene.desc.camera, W, H, collect_stats=2)
                fr.coop_threshold = coop
                img, _ = ctx.render(fr)
                assert np.array_equal(img.view(np.uint32), cnt.view(np.uint32)), "fast (bounds %d) and counting variants differ" % on
            imgs[on] = sum(c["rays"] for k, c in ctx.touched().items() if k.startswith("k_trace2"))
        assert imgs[1] < imgs[0], "the masks kept no shadow ray out of stage 2 (%d vs %d)" % (imgs[1], imgs[0])
        check_against(img, cpu, orc)
    finally:
        ctx.close()


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p11_240x135", "p4_240x135", "p7_200x150"])
def test_tile_occupancy_changes_nothing_but_the_work(pkg, ctx, golden, tag):
    """k_tile_occ: one bit per 8x8 tile of the shard and camera — can any pixel of it lie inside a node's screen rectangle (and a
    marked tile of a mesh's coverage mask)? k_primary writes the background of the other tiles without a look at cameras,
    rectangles or masks. Same bits with the shortcut on and off (rtu_debug_flags 256): ragged sizes (edge tiles, a 1x1 image),
    three shards (the shard's own tile index against the image's), a batch of turned cameras; and the counting variant."""
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    try:
        for (W, H) in [(g.width, g.height), (61, 45), (1, 1), (131, 77)]:
            res = {}
            for flag in (0, 256):
                assert pkg.hip.rtu_debug_flags(ctx._h, flag) == 0
                imgs = [render_gpu(pkg, ctx, scene, W, H, stats=False, shard_count=n)[0] for n in (1, 3)]
                cams = []
                for i in range(3):
                    cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
                    cam.pos[0] += 2.1 * i
                    cam.fov += 11.0 * i
                    cams.append(cam)
                d = pkg.hip.rtu_device_alloc(ctx._h, 3 * W * H * 16)
                ctx.render_frames_device([pkg.frame_setup(c, W, H) for c in cams], d, None)
                ctx.frame_status()
                out = np.empty((3, H, W, 4), np.float32)
                assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
                pkg.hip.rtu_device_free(ctx._h, d)
                res[flag] = imgs + [out]
            for a, b in zip(res[0], res[256]):
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), "tile occupancy changed the image at %dx%d" % (W, H)
            assert np.array_equal(res[0][0].view(np.uint32), res[0][1].view(np.uint32))
            cnt, _ = render_gpu(pkg, ctx, scene, W, H, stats=True)
            assert np.array_equal(res[0][0].view(np.uint32), cnt.view(np.uint32)), "fast and counting variants differ at %dx%d" % (W, H)
    finally:
        pkg.hip.rtu_debug_flags(ctx._h, 0)


def test_stage2_grids_from_the_last_launch_are_only_a_hint(pkg, ctx, golden):
    """The stage-2 kernel of a phase that found no work last time is launched with a smaller grid (KernelArgs::list_n). A view far
    from the mesh (short lists: the cooperative kernel's) followed by one close to it (long lists: the one-lane-per-ray
    kernel's, now on the small grid) and back again (the cooperative kernel on its token grid): every image equals the counting
    variant's, which takes no hints."""
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = 320, 200
    far = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
    near = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
    for i in range(3):
        far.pos[i] = scene.desc.camera.pos[i] * 3.0
    near.fov = 12.0
    near.dir[0], near.dir[1], near.dir[2] = 2.5 - near.pos[0], -8.0 - near.pos[1], 1.5 - near.pos[2]  # at the teapot
    ref = {}
    for name, cam in (("far", far), ("near", near)):
        ref[name], _ = ctx.render(pkg.frame_setup(cam, W, H, collect_stats=True), stats=True)
    counts = {}
    for name, cam in (("far", far), ("near", near), ("far", far), ("near", near)):
        fr = pkg.frame_setup(cam, W, H)
        fr.coop_threshold = 600
        img, _ = ctx.render(fr)  # (the synchronous entry reads the counters afterwards: the next launch of this shape takes its hints from them)
        assert np.array_equal(img.view(np.uint32), ref[name].view(np.uint32)), "stale grid hints changed the %s view" % name
        counts[name] = ctx.frame_counts()[1]
    assert max(counts["far"]) < 600 and max(counts["near"]) > 1200, "the two views do not straddle the threshold: %s" % counts


def test_materials_without_a_specular_colour_skip_the_highlight_exactly(pkg, orc, tmp_path):
    """k_consume leaves out half vector, N.H and powf for a material whose specular colour is +-0 — the second factor of a
    light's term is then `diffuse` bit for bit, PROVIDED pow() is finite. Where that does not hold the literal path must be
    taken: a light straight behind the surface point as seen from the camera (V + L = 0: the reference's half vector is 0/0
    and the pixel NaN — odd resolution, camera on the axis, so the centre pixel is that case), a negative or an absurd
    glossiness (pow infinite), a diffuse channel of -0. Fast variant == counting variant (which always takes the literal
    path) == oracle, NaN pixels included; with one camera and with a batch."""
    xml = tmp_path / "nospec.xml"
    xml.write_text("""<xml><scene>
      <object type="plane" name="floor" material="matte"><scale value="9"/></object>
      <object type="sphere" name="s1" material="neg"><scale value="1.2"/><translate x="-4" y="3" z="1.2"/></object>
      <object type="sphere" name="s2" material="huge"><scale value="1.2"/><translate x="4" y="3" z="1.2"/></object>
      <object type="sphere" name="s3" material="mzero"><scale value="1.2"/><translate x="-4" y="-3" z="1.2"/></object>
      <object type="sphere" name="s4" material="shiny"><scale value="1.2"/><translate x="4" y="-3" z="1.2"/></object>
      <object type="sphere" name="s5" material="matte"><scale value="1.0"/><translate x="0" y="4" z="1.0"/></object>
      <material type="blinn" name="matte"><diffuse r="0.7" g="0" b="0.4"/><specular value="0"/><glossiness value="25"/></material>
      <material type="blinn" name="neg"><diffuse r="0.2" g="0.6" b="0.3"/><specular value="0"/><glossiness value="-3"/></material>
      <material type="blinn" name="huge"><diffuse r="0.6" g="0.6" b="0.1"/><specular value="0"/><glossiness value="1e30"/></material>
      <material type="blinn" name="mzero"><diffuse r="-0.0" g="0.5" b="-0.0"/><specular r="-0.0" g="0" b="0"/><glossiness value="10"/></material>
      <material type="blinn" name="shiny"><diffuse r="0.3" g="0.3" b="0.6"/><specular value="0.8"/><glossiness value="40"/></material>
      <light type="ambient" name="a"><intensity value="0.1"/></light>
      <light type="point" name="below"><intensity value="40"/><position x="0" y="0" z="-10"/></light>
      <light type="point" name="atcam"><intensity value="60"/><position x="0" y="0" z="10"/></light>
      <light type="direct" name="d"><intensity value="0.5"/><direction x="0.3" y="0.2" z="-1"/></light>
    </scene><camera><position x="0" y="0" z="10"/><target x="0" y="0" z="0"/><up x="0" y="1" z="0"/><fov value="60"/>
      <width value="101"/><height value="101"/></camera></xml>""")
    scene = pkg.Scene.from_xml(str(xml))
    W, H = 101, 101
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        cpu, cst = orc.render(scene, W, H, threads=8)
        cnt, gst = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
        assert gst == cst
        check_against(cnt, cpu, orc)
        assert np.isnan(cpu[H // 2, W // 2, :3]).all(), "the centre pixel (light straight behind the floor) is not the 0/0 case any more"
        fast, _ = ctx.render(pkg.frame_setup(scene.desc.camera, W, H))
        same = (fast.view(np.uint32) == cnt.view(np.uint32)) | (np.isnan(fast) & np.isnan(cnt))
        assert same.all(), "fast and counting variants differ at %d values" % int((~same).sum())
        assert np.array_equal(np.isnan(fast), np.isnan(cnt))
        d = pkg.hip.rtu_device_alloc(ctx._h, 2 * W * H * 16)
        for attempt in range(8):
            ctx.render_frames_device([pkg.frame_setup(scene.desc.camera, W, H)] * 2, d, None)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as e:
                assert e.code == pkg.RTU_ERR_CAPACITY
        out = np.empty((2, H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
        pkg.hip.rtu_device_free(ctx._h, d)
        for i in range(2):
            same = (out[i].view(np.uint32) == cnt.view(np.uint32)) | (np.isnan(out[i]) & np.isnan(cnt))
            assert same.all()
    finally:
        ctx.close()


def test_plane_coverage_masks_in_awkward_views(pkg, orc, tmp_path):
    """k_plane_cover projects a Plane node's unit square itself (its screen rectangle is mostly air when the square is seen at an
    angle) and k_primary skips the node in tiles the projection cannot reach. Where the argument is thinnest: a square seen
    almost edge-on (no inside: only its bounding box decides), squares under nested non-uniform scales and a shear-like chain
    (parallelograms, one of them a sliver: mask unusable), a square with a corner behind the camera (unusable), a camera a hair
    above a square's edge, pixels along the squares' edges at a ragged resolution. Fast variant == counting variant (which uses
    neither rectangles nor masks) == oracle, one camera at a time and as a batch."""
    xml = tmp_path / "planes.xml"
    xml.write_text("""<xml><scene>
      <object type="plane" name="floor" material="a"><scale value="6"/><rotate angle="-45" z="1"/><translate x="1" y="2" z="0"/></object>
      <object name="g1"><scale x="1.8" y="0.6" z="1"/><rotate angle="35" z="1"/><rotate angle="20" x="1"/><translate x="-3" y="1" z="2"/>
        <object type="plane" name="tilted" material="b"><scale x="0.4" y="2.5" z="1"/><rotate angle="50" z="1"/><rotate angle="-30" y="1"/></object>
      </object>
      <object name="g2"><scale x="3" y="0.05" z="1"/><rotate angle="44" z="1"/><translate x="3" y="-1" z="1"/>
        <object type="plane" name="sliver" material="c"><rotate angle="45.5" z="1"/><scale x="1" y="14" z="1"/></object>
      </object>
      <object type="plane" name="wall" material="c"><scale value="4"/><rotate angle="90" x="1"/><translate x="0" y="9" z="3"/></object>
      <object type="sphere" name="ball" material="g"><scale value="1.1"/><translate x="0.5" y="1.5" z="1.1"/></object>
      <material type="blinn" name="a"><diffuse r="0.7" g="0.7" b="0.5"/><specular value="0"/></material>
      <material type="blinn" name="b"><diffuse r="0.3" g="0.6" b="0.8"/><specular value="0.5"/><glossiness value="30"/><reflection value="0.3"/></material>
      <material type="blinn" name="c"><diffuse r="0.8" g="0.3" b="0.3"/><specular value="0.2"/><glossiness value="10"/></material>
      <material type="blinn" name="g"><diffuse value="0.05"/><specular value="0.8"/><glossiness value="60"/><refraction index="1.4" value="0.9"/></material>
      <light type="ambient" name="amb"><intensity value="0.15"/></light>
      <light type="point" name="p"><intensity value="120"/><position x="-2" y="-6" z="12"/></light>
      <light type="direct" name="d"><intensity value="0.6"/><direction x="0.4" y="0.5" z="-1"/></light>
    </scene><camera><position x="0" y="-16" z="5"/><target x="0" y="1" z="1"/><up x="0" y="0" z="1"/><fov value="48"/>
      <width value="171"/><height value="113"/></camera></xml>""")
    scene = pkg.Scene.from_xml(str(xml))
    W, H = 171, 113
    views = [((0, -16, 5), (0, 1, 1)),            # all squares in view
             ((0, -16, 0.02), (0, 1, 0.02)),      # the floor almost edge-on
             ((1, 2, 14), (1.001, 2.001, 0)),     # straight down at the floor
             ((0.5, -3.0, 0.4), (1, 2, 0.2)),     # over the floor: corners behind the camera
             ((1 + 6 * 0.7071 + 0.01, 2 + 0.0, 0.05), (1, 2, 0)),  # a hair above and beyond a corner of the floor
             ((-9, -4, 6), (-3, 1, 2))]           # towards the tilted parallelogram
    cams = []
    for pos, tgt in views:
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        d = [t - p for p, t in zip(pos, tgt)]
        for i in range(3):
            cam.pos[i] = pos[i]
            cam.dir[i] = d[i]
        cams.append(cam)
    ctx = pkg.Context(0)
    try:
        ctx.upload(scene)
        refs = []
        for i, cam in enumerate(cams):
            cnt, gst = ctx.render(pkg.frame_setup(cam, W, H, collect_stats=True), stats=True)
            if i in (0, 3):
                s2 = pkg.Scene.from_xml(str(xml))
                for k in range(3):
                    s2.desc.camera.pos[k], s2.desc.camera.dir[k] = cam.pos[k], cam.dir[k]
                cpu, cst = orc.render(s2, W, H, threads=8)
                check_against(cnt, cpu, orc)
                assert gst == cst
            fast, _ = ctx.render(pkg.frame_setup(cam, W, H))
            assert np.array_equal(fast.view(np.uint32), cnt.view(np.uint32)), "view %d: fast and counting variants differ" % i
            refs.append(cnt)
        d = pkg.hip.rtu_device_alloc(ctx._h, len(cams) * W * H * 16)
        for attempt in range(17):
            ctx.render_frames_device([pkg.frame_setup(c, W, H) for c in cams], d, None)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as e:
                assert e.code == pkg.RTU_ERR_CAPACITY and attempt < 16
        out = np.empty((len(cams), H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
        pkg.hip.rtu_device_free(ctx._h, d)
        for i in range(len(cams)):
            assert np.array_equal(out[i].view(np.uint32), refs[i].view(np.uint32)), "batch: view %d differs" % i
    finally:
        ctx.close()


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p11_240x135", "p4_240x135", "p7_200x150", "p13_200x150", "mtl_160x120"])
def test_childless_shade_calls_settled_without_a_frame(pkg, ctx, golden, tag):
    """Round 3: a Shade() call that fires no secondary ray (mtlFunctions.cpp:125-155 and nothing else) is settled by the lane that
    found the hit — its shadow rays through the occluder lists, its light loop — and never becomes a frame record
    (render_impl.h shadows_inline). rtu_debug_flags 2048 switches that off: every image must be the same bit for bit (one frame,
    frames in flight, both stage-2 forms), the level-0 frame count must drop, and the counting variant — which always materialises
    every call — must agree with both."""
    g = golden(tag)
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    cnt, _ = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
    cams = []
    for i in range(3):
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        cam.pos[0] += 0.3 * i
        cams.append(cam)
    d = pkg.hip.rtu_device_alloc(ctx._h, 3 * W * H * 16)
    res = {}
    try:
        for flags in (0, 2048):
            pkg.hip.rtu_debug_flags(ctx._h, flags)
            for coop in (1, 10 ** 9):
                fr = pkg.frame_setup(scene.desc.camera, W, H)
                fr.coop_threshold = coop
                img, _ = ctx.render(fr)
                assert np.array_equal(img.view(np.uint32), cnt.view(np.uint32)), "flags %d, threshold %d: differs from the counting variant" % (flags, coop)
                frames, _ = ctx.frame_counts()
                res[(flags, coop)] = frames[0]
                fs = [pkg.frame_setup(c, W, H) for c in cams]
                for f in fs:
                    f.coop_threshold = coop
                for attempt in range(8):  # (a level may have to grow its frame records first: rtu_frame_status says so, render again)
                    ctx.render_frames_device(fs, d, None)
                    try:
                        ctx.frame_status()
                        break
                    except pkg.RtuError as e:
                        if e.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                            raise
                out = np.empty((3, H, W, 4), np.float32)
                assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
                res[(flags, coop, "batch")] = out
        for coop in (1, 10 ** 9):
            assert np.array_equal(res[(0, coop, "batch")].view(np.uint32), res[(2048, coop, "batch")].view(np.uint32))
            assert res[(0, coop)] <= res[(2048, coop)]
            if tag in ("teapot2_240x135", "p11_240x135"):  # (scenes whose every material reflects or refracts have no childless call)
                assert res[(0, coop)] < res[(2048, coop)], "no Shade() call was settled without a frame (%d vs %d level-0 frames)" % (res[(0, coop)], res[(2048, coop)])
    finally:
        pkg.hip.rtu_debug_flags(ctx._h, 0)
        pkg.hip.rtu_device_free(ctx._h, d)


def test_alternating_launch_shapes_do_not_reallocate(pkg, ctx, golden):
    """A caller that alternates launch shapes — a run of batches whose last one is shorter — must not make the frame arrays swing between
    the shapes' wishes: the smaller batch (below the 16 M pixels from which deeper levels start at a quarter of level 0) wants MORE at the
    deep levels and less at level 0 than the larger one. The arrays only grow (ensure_levels); found as a 2.4 s stall per timed region of
    `bench.py --frames-in-flight 24` (every launch freed and allocated 20 GB). Timed with two orders of magnitude to spare, and the
    library's own device allocations counted (rtu_debug_device_allocations): none."""
    import time
    g = golden("teapot2_1080")
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H = g.width, g.height
    big, small = 9, 8  # 18.7 M pixels (quarter rule) and 16.6 M (not)
    d = pkg.hip.rtu_device_alloc(ctx._h, big * W * H * 16)
    single = ctx.render(pkg.frame_setup(scene.desc.camera, W, H))[0]

    def launch(n):
        fs = [pkg.frame_setup(scene.desc.camera, W, H) for _ in range(n)]
        for attempt in range(8):
            ctx.render_frames_device(fs, d, None)
            try:
                ctx.frame_status()
                return
            except pkg.RtuError as e:
                if e.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                    raise
    try:
        for _ in range(2):
            launch(big)
            launch(small)
        allocs = pkg.hip.rtu_debug_device_allocations()
        t0 = time.perf_counter()
        for _ in range(6):
            launch(big)
            launch(small)
        el = time.perf_counter() - t0
        assert el < 0.6, "twelve launches took %.2f s: the frame arrays are being reallocated" % el
        grown = pkg.hip.rtu_debug_device_allocations() - allocs
        assert grown == 0, "twelve launches made %d device allocations" % grown
        got = np.empty((small, H, W, 4), np.float32)
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
        assert np.array_equal(got[small - 1].view(np.uint32), single.view(np.uint32))
    finally:
        pkg.hip.rtu_device_free(ctx._h, d)


def test_grid_hints_change_no_pixel(pkg, ctx, golden):
    """k_primary's grid follows two hints — the occupied tiles the last launch of the shape counted (k_tile_occ) and the number of launch
    sequences the caller says it keeps in flight (rtu_set_sequences_in_flight) —: 32768 / 4096 / 2048 / 1024 workgroups, tiles strided
    over them. Every combination renders the single frames' images, bit for bit; a bad argument is an error code."""
    g = golden("teapot2_1080")
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H, n = g.width, g.height, 3
    cams = []
    for i in range(n):
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        cam.pos[0] += 0.4 * i
        cams.append(cam)
    singles = [ctx.render(pkg.frame_setup(c, W, H))[0] for c in cams]
    assert sha256(singles[0][..., 3]) == g.meta["sha256_z_f32"]
    d = pkg.hip.rtu_device_alloc(ctx._h, n * W * H * 16)
    got = np.empty((n, H, W, 4), np.float32)
    try:
        assert pkg.hip.rtu_set_sequences_in_flight(ctx._h, 0) == pkg.RTU_ERR_ARG
        for seqs in (1, 2, 3, 7):
            assert pkg.hip.rtu_set_sequences_in_flight(ctx._h, seqs) == 0
            for rep in range(2):  # (the second launch of the shape knows the first's tile count)
                fs = [pkg.frame_setup(c, W, H) for c in cams]
                for attempt in range(8):
                    ctx.render_frames_device(fs, d, None)
                    try:
                        ctx.frame_status()
                        break
                    except pkg.RtuError as e:
                        if e.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                            raise
                assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
                for i in range(n):
                    assert np.array_equal(got[i].view(np.uint32), singles[i].view(np.uint32)), "sequences %d, launch %d: frame %d differs" % (seqs, rep, i)
            out = ctx.render(pkg.frame_setup(cams[1], W, H))[0]
            assert np.array_equal(out.view(np.uint32), singles[1].view(np.uint32))
    finally:
        pkg.hip.rtu_set_sequences_in_flight(ctx._h, 1)
        pkg.hip.rtu_device_free(ctx._h, d)


def test_walk_units_diagnostic_touches_only_what_it_says(pkg, ctx, golden):
    """rtu_debug_flags 131072 (include/rtu_render.h): in touched-bytes mode the one-lane-per-ray stage 2 of the primary phase writes the work
    of each deferred ray's BVH walk over the pixel's RED channel — z, green and blue of every pixel and all of the other pixels stay the
    image's; without touched-bytes mode the flag does nothing at all. The units are what the touched table counts: two per inner step of
    the 4-wide tree and one per triangle test of k_primary2, less the entries its inline shading tests."""
    g = golden("teapot2_1080")
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H, n = g.width, g.height, 4
    d = pkg.hip.rtu_device_alloc(ctx._h, n * W * H * 16)
    out = np.empty((n, H, W, 4), np.float32)

    def render(stats):
        fs = [pkg.frame_setup(scene.desc.camera, W, H, collect_stats=stats) for _ in range(n)]
        for attempt in range(8):
            ctx.render_frames_device(fs, d, None)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as e:
                if e.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                    raise
        assert pkg.hip.rtu_copy_to_host(ctx._h, out.ctypes.data, d, out.nbytes) == 0
        return out.copy()
    try:
        pkg.hip.rtu_debug_flags(ctx._h, 8192)
        ref = render(2)
        assert sha256(ref[0][..., 3]) == g.meta["sha256_z_f32"]
        pkg.hip.rtu_debug_flags(ctx._h, 8192 | 131072)
        assert np.array_equal(render(0).view(np.uint32), ref.view(np.uint32))  # not touched-bytes mode: no effect
        got = render(2)
        t = ctx.touched(False)
        assert np.array_equal(got[..., 1:].view(np.uint32), ref[..., 1:].view(np.uint32))
        changed = got[0, ..., 0] != ref[0, ..., 0]
        _, deferred = ctx.frame_counts()
        assert 0.97 * deferred[0] / n <= changed.sum() <= deferred[0] / n  # (a unit count may coincide with the red it replaces)
        units = got[0, ..., 0][changed]
        assert units.min() >= 1 and units.max() < 1000 and np.all(units == np.round(units))
        k2 = t["k_primary2"]
        assert abs(n * units.sum() - (2 * k2["inner4"] + k2["tri_tests"])) <= 0.2 * n * units.sum()  # (+ the list entries of the inline shading)
    finally:
        pkg.hip.rtu_debug_flags(ctx._h, 0)
        pkg.hip.rtu_device_free(ctx._h, d)


def test_idle_cooperative_launches_dropped_and_a_wrong_hint_is_harmless(pkg, ctx, golden):
    """Round 3: a phase whose list was the one-lane-per-ray kernel's last time launches no (idle) cooperative kernel — its workgroups
    want a whole CU and stall the sequence beside another stream's kernels — and the one-lane-per-ray kernel takes the list WHATEVER
    its length turns out to be. So a batch of the same shape whose lists are short this time (the cameras moved away) is rendered
    by the kernel the hint chose, not the one the threshold would: the images must still be the single frames', bit for bit; and
    rtu_debug_flags 16384 (both kernels launched, as before) renders the same."""
    g = golden("teapot2_1080")
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H, n = g.width, g.height, 4

    def cams_at(scale):
        out = []
        for i in range(n):
            cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
            for k in range(3):
                cam.pos[k] *= scale
            cam.pos[0] += 0.5 * i
            out.append(cam)
        return out
    near, far = cams_at(1.0), cams_at(3.5)
    singles = {id(c): ctx.render(pkg.frame_setup(c, W, H))[0] for c in near + far}
    d = pkg.hip.rtu_device_alloc(ctx._h, n * W * H * 16)
    got = np.empty((n, H, W, 4), np.float32)

    def render(cams, stats=0):
        fs = [pkg.frame_setup(c, W, H, collect_stats=stats) for c in cams]
        for attempt in range(8):
            ctx.render_frames_device(fs, d, None)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as e:
                if e.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                    raise
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
        for i, c in enumerate(cams):
            assert np.array_equal(got[i].view(np.uint32), singles[id(c)].view(np.uint32)), "frame %d differs" % i
    try:
        for flags in (8192, 8192 | 16384, 0):
            pkg.hip.rtu_debug_flags(ctx._h, flags)
            render(near)
            render(near)              # the shape's hint: long lists
            _, deferred = ctx.frame_counts()
            assert deferred[0] > 70000
            render(far)               # same shape, short lists: rendered by the kernels the hint chose
            _, deferred = ctx.frame_counts()
            assert 0 < deferred[0] < 70000
            render(far)               # ... and by the ones the new hint chooses
            render(near)              # and back: the cooperative kernel's grid meets a long list
            render(near, 2)
            t = ctx.touched(False)
            assert "k_primary2" in t and "k_primary2c" not in t
    finally:
        pkg.hip.rtu_debug_flags(ctx._h, 0)
        pkg.hip.rtu_device_free(ctx._h, d)


def test_stage2_of_the_primary_phase_beside_the_recursion_levels(pkg, ctx, golden):
    """Round 3, side mode (rtu_device.h KernelArgs::fcnt0): once a launch shape has shown that stage 2 of its primary phase is the
    one-lane-per-ray kernel and makes at most a few hundred frames, that kernel runs on the context's helper stream beside the
    recursion levels, with a defer list, counters and a small set of level arrays of its own and one k_tail launch behind it.
    The images must be those of the launch-stream order (rtu_debug_flags 8192) and of the frames rendered alone, bit for bit;
    the touched-bytes table shows that the mode was in fact taken (slot k_tail(side)) and its bookkeeping still adds up."""
    g = golden("teapot2_1080")
    scene = g.scene(pkg)
    ctx.upload(scene)
    W, H, n = g.width, g.height, 4
    cams = []
    for i in range(n):
        cam = type(scene.desc.camera).from_buffer_copy(scene.desc.camera)
        cam.pos[0] += 0.6 * i
        cam.pos[2] += 0.2 * i
        cams.append(cam)
    singles = [ctx.render(pkg.frame_setup(c, W, H))[0] for c in cams]
    assert sha256(singles[0][..., 3]) == g.meta["sha256_z_f32"]
    d = pkg.hip.rtu_device_alloc(ctx._h, n * W * H * 16)
    got = np.empty((n, H, W, 4), np.float32)

    def render(stats):
        fs = [pkg.frame_setup(c, W, H, collect_stats=stats) for c in cams]
        for attempt in range(8):
            ctx.render_frames_device(fs, d, None)
            try:
                ctx.frame_status()
                break
            except pkg.RtuError as e:
                if e.code != pkg.RTU_ERR_CAPACITY or attempt == 7:
                    raise
        assert pkg.hip.rtu_copy_to_host(ctx._h, got.ctypes.data, d, got.nbytes) == 0
        return got.copy()
    try:
        for flags in (8192, 0):
            pkg.hip.rtu_debug_flags(ctx._h, flags)
            for rep in range(3):  # the first launches of a shape teach the context its habits; the third is in side mode (flags 0)
                out = render(0)
                for i in range(n):
                    assert np.array_equal(out[i].view(np.uint32), singles[i].view(np.uint32)), "flags %d, launch %d: frame %d differs" % (flags, rep, i)
            out = render(2)
            t = ctx.touched(False)
            for i in range(n):
                assert np.array_equal(out[i].view(np.uint32), singles[i].view(np.uint32)), "flags %d, touched-bytes mode: frame %d differs" % (flags, i)
            nl = (ctypes.c_uint32 * pkg.KERNEL_SLOTS)()
            n_slots = pkg.hip.rtu_get_touched_launches(ctx._h, nl, pkg.KERNEL_SLOTS)
            side = nl[[pkg.hip.rtu_kernel_slot_name(k).decode() for k in range(n_slots)].index("k_tail(side)")]
            if flags == 0:
                assert side >= 1, "side mode was not taken"
            else:
                assert side == 0 and "k_tail(side)" not in t, "side mode taken under rtu_debug_flags 8192"
                assert t.get("k_primary2", {}).get("rays", 0) > 0  # stage 2 of the primary phase in the launch stream
            if flags == 0:
                assert "k_primary2" in t and "k_primary2c" not in t  # the long list: one lane per ray
                _, deferred = ctx.frame_counts()
                walks = lambda k: t[k]["rays"] - t[k]["inline_shadow_rays"] if k in t else 0
                assert walks("k_primary") == n * W * H and walks("k_primary2") == deferred[0] > 70000
    finally:
        pkg.hip.rtu_debug_flags(ctx._h, 0)
        pkg.hip.rtu_device_free(ctx._h, d)
