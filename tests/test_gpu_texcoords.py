"""Texture coordinates at their discontinuities, device against the oracle.

A checkerboard is a discrete decision (u <= 0.5 after the map transform, the wrap at integers in TileClamp), and so is
the texel of a file texture: one ulp of u on a pixel that sits on an edge is a whole colour, not a level of RGB. The
inputs of those decisions come from atan2f / asinf (sphere uv, environment direction) and from int(float) casts.
The function-level tests run the kernels' own __device__ functions through rtu_debug_texcoords and compare them bit
for bit with the oracle's (libm's atan2f / asinf, x86 int casts); the scene-level tests put many pixels on edges at
1080p and 4K and hold them to the usual bars (test_gpu_parity.check_against)."""
import ctypes
import itertools
import math

import numpy as np
import pytest

from test_gpu_parity import check_against
from test_gpu_sampled import check as check_sampled

pytestmark = pytest.mark.gpu

CHUNK = 1 << 24  # inputs per round trip: a few hundred MB of host memory at most


@pytest.fixture(scope="module")
def ctx(pkg):
    c = pkg.Context(0)
    yield c
    c.close()


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def differing(a, b):
    """Results that differ in any bit; two NaNs are equal (the sign and payload of a NaN are not part of the contract)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    bad = a.view(np.uint32) != b.view(np.uint32)
    bad &= ~(np.isnan(a) & np.isnan(b))
    return bad.reshape(bad.shape[0], -1).any(axis=1) if bad.ndim > 1 else bad


def compare(pkg, orc, ctx, op, x, what, index=0, scene=None):
    """Device against oracle on the inputs x ([n, TEXOP_IN[op]], or an iterable of such arrays, each made when it is
    compared), in chunks of CHUNK; asserts no input differs."""
    if isinstance(x, np.ndarray):
        arr = np.ascontiguousarray(x, np.float32).reshape(-1, pkg.TEXOP_IN[op])
        x = (arr[s:s + CHUNK] for s in range(0, len(arr), CHUNK))
    nbad, total, first = 0, 0, None
    for xs in x:
        xs = np.ascontiguousarray(xs, np.float32).reshape(-1, pkg.TEXOP_IN[op])
        bad = differing(ctx.texcoords(op, xs, index), orc.texcoords(op, xs, index, scene, threads=16))
        if bad.any() and first is None:
            first = xs[np.argmax(bad)]
        nbad += int(bad.sum())
        total += len(xs)
    print("%s: %d of %d inputs differ" % (what, nbad, total))
    assert nbad == 0, "%s: %d of %d inputs differ from the oracle (first: %r)" % (what, nbad, total, first)


def unit_vectors(rng, n):
    """Normals as the kernels make them: a float vector divided by its float length."""
    v = rng.random((n, 3), dtype=np.float32) * np.float32(2) - np.float32(1)
    return v / np.sqrt((v * v).sum(axis=1, dtype=np.float32))[:, None]


def unit_vector_chunks(rng, n):
    for _ in range(n // (CHUNK // 4)):
        yield unit_vectors(rng, CHUNK // 4)


def axis_vectors():
    """Signed axes, signed zeros, diagonals and near-axis vectors, among them (0, 0, +-1) and (+-0, +-0, +-1)."""
    z, o, e, d = 0.0, 1.0, 1e-30, np.float32(1 / math.sqrt(2))
    vals = []
    for a in (z, -z, o, -o, e, -e, d, -d, np.float32(1 / math.sqrt(3)), -np.float32(1 / math.sqrt(3)), f32(1).item(), -f32(1).item()):
        for b in (z, -z, o, -o, e, -e, d, -d, np.float32(1 / math.sqrt(3)), f32(1).item()):
            for c in (z, -z, o, -o, d, -d, np.float32(1 / math.sqrt(3)), f32(0x3f7fffff).item()):
                vals.append((a, b, c))
    return np.array(vals, np.float32)


def extremes():
    """Where int(float) and TileClamp go wrong: signed zeros, exact integers, just below 0 (u + 1 rounds to 1), +-2^31 and
    beyond, +-inf, NaN, subnormals."""
    v = [0.0, -0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0, 3.0, -7.0, 1e-45, -1e-45, 1e-38, -1e-38, -1e-8, -3e-8, -6e-8, -1e-30,
         f32(0xbf7fffff).item(), f32(0x3f7fffff).item(), f32(0xb3800000).item(), f32(0xb3000000).item(), 1 - 2 ** -24, -(1 - 2 ** -24),
         2 ** 23, 2 ** 23 + 1, 2 ** 24, -2 ** 24, 2 ** 30, -2 ** 30, 2147483520.0, -2147483520.0, 2 ** 31, -2 ** 31,
         f32(0xcf000001).item(), f32(0x4f000001).item(), 3e9, -3e9, 4294967296.0, 1e20, -1e20, 3.4e38, -3.4e38,
         math.inf, -math.inf, math.nan, -math.nan, 0.49999997, 0.50000006, 1.5, -1.5, 0.25, 0.75]
    return np.array(v, np.float32)


def triples(vals, rng, n_random=0):
    """Every (a, b, c) of the values for a and b, c cycling, plus random combinations."""
    a, b = np.meshgrid(vals, vals, indexing="ij")
    c = np.resize(vals, a.size)
    t = np.stack([a.ravel(), b.ravel(), c], axis=1)
    if n_random:
        t = np.concatenate([t, rng.choice(vals, (n_random, 3))])
    return t.astype(np.float32)


def test_asinf(pkg, orc, ctx):
    """asinf as the kernels call it, against the host libm's: every 8th float of [-1, 1] (267 million), all of the last
    65536 floats below 1, the first floats above 0, the subnormals' edges, +-0, +-1 and the values just outside.
    Each chunk of bit patterns is made when it is compared."""
    def chunks():
        for sign in (np.uint32(0), np.uint32(0x80000000)):
            for start in range(0, 0x3f800001, 8 * CHUNK):
                yield f32(np.arange(start, min(start + 8 * CHUNK, 0x3f800001), 8, dtype=np.uint32) | sign)
            yield f32(np.concatenate([np.arange(0x3f800000 - 65536, 0x3f800008, dtype=np.uint32), np.arange(0, 65536, dtype=np.uint32),
                                      np.arange(0x007f0000, 0x00810000, dtype=np.uint32)]) | sign)
    compare(pkg, orc, ctx, pkg.TEXOP_ASINF, chunks(), "asinf")


def test_atan2f_unit_vectors(pkg, orc, ctx):
    """atan2f on 2^28 pairs (N.x, N.y) of random unit normals, and of unit vectors of the xy plane."""
    rng = np.random.default_rng(7)
    nbad, total = 0, 0
    for k in range(16):
        n = unit_vectors(rng, 1 << 24)
        if k % 4 == 3:  # in the xy plane: |N.x| and |N.y| near 1, atanf's reduction at its largest arguments
            n = n[:, :2] / np.sqrt((n[:, :2] * n[:, :2]).sum(axis=1, dtype=np.float32))[:, None]
        yx = np.ascontiguousarray(n[:, :2])
        bad = differing(ctx.texcoords(pkg.TEXOP_ATAN2F, yx), orc.texcoords(pkg.TEXOP_ATAN2F, yx, threads=16))
        nbad += int(bad.sum())
        total += len(yx)
    print("atan2f unit vectors: %d of %d pairs differ" % (nbad, total))
    assert nbad == 0, "atan2f: %d of %d pairs differ from the oracle" % (nbad, total)


def test_atan2f_special_cases(pkg, orc, ctx):
    """atan2f on every pair of signed zeros, axes, diagonals, subnormals, +-inf, NaN, huge and tiny ratios (the
    |y/x| = 2^+-60 cut-offs), and on random bit patterns of both operands."""
    v = [0.0, -0.0, 1.0, -1.0, 1e-45, -1e-45, 1e-40, -1e-40, 1.17549435e-38, -1.17549435e-38, 2.0, -2.0, 0.5, 0.70710677,
         -0.70710677, 0.70710683, 1 - 2 ** -24, 1 + 2 ** -23, 0.4375, 1.1875, 2.4375, 2 ** 25, 2 ** 60, 2 ** -60, 2 ** 61,
         2 ** -61, 2 ** 62, 3e38, -3e38, math.inf, -math.inf, math.nan, 3.0, 7.0]
    v = np.array(v, np.float32)
    a, b = np.meshgrid(v, v, indexing="ij")
    pairs = np.stack([a.ravel(), b.ravel()], axis=1)
    rng = np.random.default_rng(3)
    rnd = f32(rng.integers(0, 1 << 32, (1 << 22, 2), dtype=np.uint64).astype(np.uint32))
    compare(pkg, orc, ctx, pkg.TEXOP_ATAN2F, np.concatenate([pairs, rnd]), "atan2f special")


def test_sphere_uv(pkg, orc, ctx):
    """Sphere::IntersectRay's uv (the helper every sphere test of every kernel calls) on 2^24 random unit normals and
    on axes, signed zeros and diagonals."""
    rng = np.random.default_rng(11)
    compare(pkg, orc, ctx, pkg.TEXOP_SPHERE_UV, itertools.chain([axis_vectors()], unit_vector_chunks(rng, 1 << 24)), "sphere uv")


def test_env_uvw(pkg, orc, ctx):
    """SampleEnvironment's uvw on 2^24 random unit directions and on axes, among them (0, 0, +-1) where x / y is 0 / 0."""
    rng = np.random.default_rng(13)
    compare(pkg, orc, ctx, pkg.TEXOP_ENV_UVW, itertools.chain([axis_vectors()], unit_vector_chunks(rng, 1 << 24)), "environment uvw")


def test_tile_clamp(pkg, orc, ctx):
    """TileClamp at -0, exact integers, just below 0, +-2^31 and beyond, +-inf and NaN: x86's int(float) (INT_MIN for NaN
    and out of range) is the reference's."""
    rng = np.random.default_rng(17)
    x = np.concatenate([triples(extremes(), rng, 1 << 16), rng.uniform(-3e9, 3e9, (1 << 16, 3)).astype(np.float32)])
    compare(pkg, orc, ctx, pkg.TEXOP_TILE_CLAMP, x, "tile_clamp")
    # the x86 result, pinned: the oracle is the reference's arithmetic on its platform
    out = orc.texcoords(pkg.TEXOP_TILE_CLAMP, np.array([[3e9, -3e9, math.nan]], np.float32))
    assert out[0, 0] == np.float32(3e9) + np.float32(2 ** 31) and out[0, 1] == np.float32(-3e9) + np.float32(2 ** 31) and np.isnan(out[0, 2])


class _Tex(ctypes.Structure):  # RtuTexture, include/rtu_scene.h
    _fields_ = [("type", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("rgb", ctypes.c_void_p), ("color1", ctypes.c_float * 3), ("color2", ctypes.c_float * 3)]


def _ppm(path, w, h, seed):
    rnd = np.random.default_rng(seed)
    path.write_bytes(b"P6\n%d %d\n255\n" % (w, h) + rnd.integers(0, 256, w * h * 3, dtype=np.uint8).tobytes())


TEX_MATERIALS = """
      <material type="blinn" name="c1"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.1" g="0.2" b="0.3"/><color2 r="0.9" g="0.8" b="0.7"/></diffuse></material>
      <material type="blinn" name="c2"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0" g="0" b="0"/><color2 r="1" g="1" b="1"/>
        <scale value="0.001"/></diffuse><specular r="1" g="1" b="1" texture="checkerboard"><color1 r="0.3" g="0" b="0"/><color2 r="0" g="0.3" b="0"/><scale x="0.06" y="0.07"/><rotate angle="30" z="1"/></specular></material>
      <material type="blinn" name="f1"><diffuse texture="{d}/row.ppm"/><specular texture="{d}/wide.ppm"><scale x="1e-6" y="3"/><translate x="0.25"/></specular></material>
      <material type="blinn" name="f2"><diffuse texture="{d}/wide.ppm"/><specular texture="{d}/col.ppm"/></material>"""


def _texture_scene(pkg, tmp_path):
    _ppm(tmp_path / "row.ppm", 7, 1, 1)    # 1 x N: every sample wraps in y
    _ppm(tmp_path / "col.ppm", 1, 5, 2)
    _ppm(tmp_path / "wide.ppm", 13, 5, 3)  # non-square
    xml = tmp_path / "tex.xml"
    xml.write_text("""<xml><scene>
      <background r="1" g="1" b="1" texture="checkerboard"><color1 r="0" g="0" b="0"/><color2 r="1" g="1" b="1"/><scale value="0.02"/></background>
      <environment value="1" texture="{d}/wide.ppm"><scale value="0.5"/><rotate angle="10" z="1"/></environment>
      <object type="sphere" name="a" material="c1"/><object type="sphere" name="b" material="c2"><translate x="3"/></object>
      <object type="sphere" name="c" material="f1"><translate y="3"/></object><object type="sphere" name="d" material="f2"><translate y="-3"/></object>
      {m}
      <light type="ambient" name="a"><intensity value="0.2"/></light>
    </scene><camera><position x="0" y="-10" z="0"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="40"/>
      <width value="64"/><height value="48"/></camera></xml>""".format(d=tmp_path, m=TEX_MATERIALS.format(d=tmp_path)))
    return pkg.Scene.from_xml(str(xml))


def _sample_points(tex, rng):
    """u exactly 0.5, texel boundaries and their neighbours, the int(float) extremes, random points."""
    w, h = max(tex.width, 2), max(tex.height, 2)
    edges = np.unique(np.concatenate([np.arange(-2 * w, 2 * w + 1) / np.float32(w), np.arange(-2 * h, 2 * h + 1) / np.float32(h),
                                      np.arange(-8, 9) / np.float32(4)]).astype(np.float32))
    near = np.concatenate([edges, np.nextafter(edges, np.float32(-np.inf)), np.nextafter(edges, np.float32(np.inf))])
    vals = np.unique(np.concatenate([near, extremes()]))
    return np.concatenate([triples(vals, rng, 1 << 16), rng.uniform(-20, 20, (1 << 18, 3)).astype(np.float32)])


def test_texture_sample(pkg, orc, ctx, tmp_path):
    """TextureChecker::Sample and TextureFile::Sample (bilinear, tiled) of every texture of a scene with checkers and
    1 x 7, 5 x 1 and 13 x 5 file textures: at u = 0.5, on texel boundaries and one ulp either side, at the extremes of
    TileClamp, at random points."""
    scene = _texture_scene(pkg, tmp_path)
    ctx.upload(scene)
    rng = np.random.default_rng(19)
    kinds = set()
    for i in range(scene.desc.n_textures):
        t = _Tex.from_address(scene.desc.textures + i * ctypes.sizeof(_Tex))
        kinds.add((t.type, t.width, t.height))
        compare(pkg, orc, ctx, pkg.TEXOP_TEXTURE, _sample_points(t, rng), "texture %d (%d: %dx%d)" % (i, t.type, t.width, t.height), i, scene)
    assert {(w, h) for _, w, h in kinds} >= {(7, 1), (1, 5), (13, 5)} and len({k[0] for k in kinds}) == 2, kinds


def _present_maps(pkg, scene):
    """The maps TEXOP_MAP samples: material maps (4 * material + RTU_MAP_*), background (-1), environment (-2), present or not."""
    d = scene.desc
    mats = (pkg.RtuTexMap * (4 * d.n_materials)).from_address(d.material_maps) if d.material_maps else []
    maps = {-1: d.background_map.present, -2: d.environment_map.present}
    maps.update({i: m.present for i, m in enumerate(mats)})
    return maps


def test_map_sample(pkg, orc, ctx, tmp_path):
    """TextureMap::Sample (the map's transform, then the texture) of every present material map and of the background and
    environment maps, on the same points: a map scale of 0.001 and 1e-6 multiplies an error by a million before the edge."""
    scene = _texture_scene(pkg, tmp_path)
    ctx.upload(scene)
    rng = np.random.default_rng(23)
    t = _Tex(width=13, height=5)
    x = _sample_points(t, rng)
    maps = [i for i, present in _present_maps(pkg, scene).items() if present]
    assert len(maps) == 9, maps  # background, environment and seven material maps
    for i in maps:
        compare(pkg, orc, ctx, pkg.TEXOP_MAP, x, "map %d" % i, i, scene)


def _refused(fn):
    try:
        fn()
    except Exception as e:  # RtuError / OracleError, both with .code
        return getattr(e, "code", None)
    return None


def test_texcoords_refuse_what_is_not_there(pkg, orc, ctx, golden, tmp_path):
    """TEXTURE / MAP of a scene without textures, of a map that is not present and of an index out of range are refused
    with an argument error on both sides, before any kernel reads a texture (an untextured scene has no texture array,
    and an absent map's texture index is not checked at upload)."""
    x = np.zeros((4, 3), np.float32)
    plain = golden("teapot2_240x135").scene(pkg)
    assert plain.desc.n_textures == 0
    ctx.upload(plain)
    for op, index in ((pkg.TEXOP_MAP, -1), (pkg.TEXOP_MAP, -2), (pkg.TEXOP_MAP, 0), (pkg.TEXOP_TEXTURE, 0)):
        assert _refused(lambda: ctx.texcoords(op, x, index)) == pkg.RTU_ERR_ARG, (op, index)
        assert _refused(lambda: orc.texcoords(op, x, index, plain)) == orc.ERR_ARG, (op, index)
    scene = _texture_scene(pkg, tmp_path)
    ctx.upload(scene)
    absent = [i for i, present in _present_maps(pkg, scene).items() if not present]
    assert len(absent) > 4
    for op, index in [(pkg.TEXOP_MAP, i) for i in absent] + [(pkg.TEXOP_MAP, 4 * scene.desc.n_materials), (pkg.TEXOP_MAP, -3),
                                                             (pkg.TEXOP_TEXTURE, scene.desc.n_textures), (pkg.TEXOP_TEXTURE, -1)]:
        assert _refused(lambda: ctx.texcoords(op, x, index)) == pkg.RTU_ERR_ARG, (op, index)
        assert _refused(lambda: orc.texcoords(op, x, index, scene)) == orc.ERR_ARG, (op, index)
    # the context still works afterwards
    assert ctx.texcoords(pkg.TEXOP_TEXTURE, x, 0).shape == (4, 3)


def test_upload_refuses_a_file_texture_with_one_side_zero(pkg, ctx, tmp_path):
    """A file texture of 0 x h or w x 0 would make TextureFile::Sample divide by 0 and read an image that is not there:
    the upload refuses it."""
    scene = _texture_scene(pkg, tmp_path)
    for i in range(scene.desc.n_textures):
        t = _Tex.from_address(scene.desc.textures + i * ctypes.sizeof(_Tex))
        if t.type == 0 and t.width > 1:
            w = t.width
            t.width = 0
            assert _refused(lambda: ctx.upload(scene)) == pkg.RTU_ERR_ARG
            t.width = w
    ctx.upload(scene)


# ---- scenes --------------------------------------------------------------------------------------------------------

def _render_both(pkg, ctx, scene, W, H):
    ctx.upload(scene)
    fast, _ = ctx.render(pkg.frame_setup(scene.desc.camera, W, H))
    cnt, gst = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, collect_stats=True), stats=True)
    return fast, cnt, gst


def check_scene(pkg, orc, ctx, scene, W, H, what):
    """Fast and counting variants against the oracle at the usual bars; prints how many pixels differ first."""
    fast, cnt, gst = _render_both(pkg, ctx, scene, W, H)
    cpu, cst = orc.render(scene, W, H, threads=16)
    for img, v in ((fast, "fast"), (cnt, "counting")):
        zbad = int((img[..., 3].view(np.uint32) != cpu[..., 3].view(np.uint32)).sum())
        g8, _, _ = orc.postprocess(img)
        c8, _, _ = orc.postprocess(cpu)
        d8 = np.abs(g8.astype(np.int32) - c8.astype(np.int32)).max(axis=2)
        print("%s %dx%d %s: %d pixels differ in z, %d by more than one level of RGB (max %d)" % (what, W, H, v, zbad, int((d8 > 1).sum()), int(d8.max())))
        check_against(img, cpu, orc)
    assert gst == cst, "counters differ"
    return cpu


@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160)])
def test_project7_large(pkg, orc, ctx, golden, size):
    """Project7 (checkers on a sphere and a plane, a PNG on the teapot, PNG background and environment, mirror and
    glass) at the sizes DESIGN quotes it, where many more pixels lie within an ulp of a checker edge."""
    scene = golden("p7_200x150").scene(pkg)
    check_scene(pkg, orc, ctx, scene, *size, "p7")


def _checker_xml(tmp_path, W, H, extra_light=""):
    xml = tmp_path / "checker.xml"
    xml.write_text("""<xml><scene>
      <background r="1" g="1" b="1" texture="checkerboard"><color1 r="0.1" g="0.2" b="0.3"/><color2 r="0.9" g="0.8" b="0.7"/><scale x="0.02" y="0.03"/></background>
      <environment value="1" texture="checkerboard"><color1 r="0.3" g="0.1" b="0"/><color2 r="0.9" g="0.9" b="1"/><scale value="0.05"/></environment>
      <object type="sphere" name="big" material="chk"><scale value="4"/></object>
      <object type="sphere" name="mirror" material="mirror"><scale value="2"/><translate x="4.5" y="-5" z="1.5"/></object>
      <material type="blinn" name="chk"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.05" g="0.1" b="0.6"/><color2 r="0.95" g="0.9" b="0.3"/>
        <scale x="0.06" y="0.055"/></diffuse><specular value="0.3"/><glossiness value="20"/></material>
      <material type="blinn" name="mirror"><diffuse value="0.02"/><specular value="0.2"/><glossiness value="60"/><reflection value="0.95"/></material>
      <light type="ambient" name="a"><intensity value="0.3"/></light>
      <light type="direct" name="d"><intensity value="0.7"/><direction x="-0.3" y="0.5" z="-1"/></light>{light}
    </scene><camera><position x="0" y="-16" z="0"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="34"/>
      <width value="{W}"/><height value="{H}"/></camera></xml>""".format(W=W, H=H, light=extra_light))
    return str(xml)


@pytest.mark.parametrize("size", [(1920, 1080), (3840, 2160)])
def test_checker_scene(pkg, orc, ctx, tmp_path, size):
    """A sphere filling the frame under a checker map of about a thousand cells, a mirror sphere showing a checker
    environment, a checker background: sphere uv, environment uvw and background coordinates on thousands of edges."""
    scene = pkg.Scene.from_xml(_checker_xml(tmp_path, *size))
    cpu = check_scene(pkg, orc, ctx, scene, *size, "checker")
    c8, _, _ = orc.postprocess(cpu)
    # the edges are there: many pixels of each of the two sphere colours and of the background's
    assert len(np.unique(c8.reshape(-1, 3), axis=0)) > 200


def _mirror_xml(tmp_path, env):
    return """<xml><scene>
      <background r="0" g="0" b="0"/>{env}
      <object type="plane" name="floor" material="mirror"><scale value="100"/></object>
      <material type="blinn" name="mirror"><diffuse value="0.1"/><specular value="0"/><glossiness value="10"/><reflection value="0.9"/></material>
      <light type="ambient" name="a"><intensity value="0.5"/></light>
    </scene><camera><position x="0" y="0" z="10"/><target x="0" y="0" z="0"/><up x="0" y="1" z="0"/><fov value="60"/>
      <width value="101"/><height value="75"/></camera></xml>""".format(env=env)


@pytest.mark.parametrize("env", ["file", "checker"])
@pytest.mark.parametrize("size", [(101, 75), (1921, 1081)])
def test_straight_down_mirror(pkg, orc, ctx, tmp_path, env, size):
    """A camera looking straight down at a mirror, odd resolution: the centre pixel's reflected ray is (0, 0, 1), and
    SampleEnvironment divides 0 by 0. The uvw is NaN, so the colour is NaN (file) or color1 (checker) whatever an int
    cast gives; the casts themselves are checked by test_tile_clamp and test_texture_sample."""
    _ppm(tmp_path / "env.ppm", 9, 7, 5)
    e = ('<environment value="1" texture="%s/env.ppm"/>' % tmp_path if env == "file" else
         '<environment value="1" texture="checkerboard"><color1 r="0.2" g="0.3" b="0.4"/><color2 r="0.9" g="0.7" b="0.5"/><scale value="0.1"/></environment>')
    xml = tmp_path / "mirror.xml"
    xml.write_text(_mirror_xml(tmp_path, e))
    scene = pkg.Scene.from_xml(str(xml))
    W, H = size
    cpu = check_scene(pkg, orc, ctx, scene, W, H, "mirror/" + env)
    if env == "file":  # the 0 / 0 is reached: the centre pixel's colour is NaN on both sides
        assert np.isnan(cpu[H // 2, W // 2, :3]).all()


def _huge_vt_xml(tmp_path, vts):
    obj = tmp_path / "quad.obj"
    lines = ["v -2 0 -1", "v 2 0 -1", "v 2 0 1", "v -2 0 1", "v 0 0 2"] + ["vt %s %s" % p for p in vts] + ["vn 0 -1 0"]
    lines += ["f 1/1/1 2/2/1 3/3/1", "f 1/1/1 3/3/1 4/4/1", "f 4/4/1 3/3/1 5/5/1"]
    obj.write_text("\n".join(lines) + "\n")
    _ppm(tmp_path / "tex.ppm", 11, 6, 9)
    xml = tmp_path / "vt.xml"
    xml.write_text("""<xml><scene>
      <object type="obj" name="{d}/quad.obj" material="file"><translate x="-2.2"/></object>
      <object type="obj" name="{d}/quad.obj" material="chk"><translate x="2.2"/></object>
      <material type="blinn" name="file"><diffuse texture="{d}/tex.ppm"/><specular value="0.2"/><glossiness value="10"/></material>
      <material type="blinn" name="chk"><diffuse texture="checkerboard"><color1 r="0.1" g="0.2" b="0.3"/><color2 r="0.9" g="0.8" b="0.7"/></diffuse></material>
      <light type="ambient" name="a"><intensity value="0.3"/></light><light type="direct" name="d"><intensity value="0.7"/><direction x="0.2" y="1" z="-0.3"/></light>
    </scene><camera><position x="0" y="-12" z="0.5"/><target x="0" y="0" z="0.5"/><up x="0" y="0" z="1"/><fov value="40"/>
      <width value="160"/><height value="90"/></camera></xml>""".format(d=tmp_path))
    return str(xml)


@pytest.mark.parametrize("vts", [
    [("3e9", "0.25"), ("-3e9", "0.5"), ("1e20", "0.75"), ("0.5", "3e9"), ("-1e20", "-3e9")],
    [("2147483520", "-2147483904"), ("2147483648", "0.5"), ("-2147483648", "-2147483648"), ("0.5", "1e20"), ("1e10", "1e-40")],
    [("inf", "0.5"), ("nan", "0.25"), ("-inf", "nan"), ("0.5", "inf"), ("1", "-inf")],
], ids=["huge", "int-edges", "inf-nan"])
def test_huge_texture_vertices(pkg, orc, ctx, tmp_path, vts):
    """An .obj whose vt values (read with %f) lie beyond the int range, at its edges, or are inf / nan, under a file
    texture and a checker: every int(float) of TileClamp and TextureFile::Sample on x86's INT_MIN side."""
    scene = pkg.Scene.from_xml(_huge_vt_xml(tmp_path, vts))
    for W, H in ((160, 90), (1280, 720)):
        check_scene(pkg, orc, ctx, scene, W, H, "vt " + vts[0][0])


def test_recipe_s_checker(pkg, orc, ctx, tmp_path):
    """Recipe S on the checker scene with a soft light, 4 samples: sphere uv in the sampled kernels."""
    xml = _checker_xml(tmp_path, 240, 136, '<light type="point" name="p"><intensity value="0.5"/><position x="-6" y="-10" z="8"/><size value="1.5"/></light>')
    scene = pkg.Scene.from_xml(xml)
    W, H, spp = 240, 136, 4
    cpu, cst = orc.render_samples(scene, W, H, spp, stream=orc.STREAM_KEYED, trig=orc.TRIG_PORTABLE, threads=16)
    ctx.upload(scene)
    fast, _ = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, samples=spp))
    check_sampled(fast, cpu, orc, spp, "recipe S fast")
    cnt, gst = ctx.render(pkg.frame_setup(scene.desc.camera, W, H, samples=spp, collect_stats=True), stats=True)
    assert np.array_equal(cnt.view(np.uint32), fast.view(np.uint32)), "fast and counting variants differ"
    assert gst == cst, "counters differ"
