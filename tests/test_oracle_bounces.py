"""CPU-only: the oracle at every recursion depth (RtuFrameDesc.max_bounce of the device, 0..5) against the compiled reference.

The reference passes bounceCount 5 to every root Shade() call (RenderFunctions.cpp:134-135); the oracle takes another depth through
a test hook (the max_bounce keyword of oracle_binding's render calls), the reference harness through `ref_render --bounces N`.
tests/golden/<tag>/bounce<k>.npz are the harness's images and counters at depth k (make_goldens.py bounces), on the tag's own
scene.rtus.gz. What pins the hook besides them: depth 5 through the hook is the call without it, depth 0 is the scene with every
mirror and every glass taken out rendered without the hook, and the depth-5 counters are those of each tag's meta.json.

Secondary rays at depth 0..5, and pixels (any bit of r, g or b) differing from the previous depth, recipe W at each tag's own size:

    tag               secondary rays at depth 0..5                  pixels differing from the previous depth
    p4_240x135        0, 6328, 11313, 15176, 18003, 20857           -, 3657, 2477, 1266, 1296, 1282
    p13_200x150       0, 4164, 7015, 8955, 10003, 11096             -, 1934, 1148, 412, 431, 393
    p5_200x150        0, 6338, 9857, 12337, 13706, 15131            -, 4534, 1850, 865, 669, 656
    p7_200x150        0, 23254, 33757, 41568, 44957, 46533          -, 19624, 6138, 4333, 1656, 869
    mtl_160x120       0, 12497, 34702, 65612, 118060, 231400        -, 2808, 1815, 2305, 1157, 1153
    teapot2_240x135   0, 448, 825, 978, 979, 980                    -, 61, 148, 0, 0, 0

Every depth shows in the image of five scenes; teapot2 saturates (depths 2..5 are one image while the counters still move)."""
import glob
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

TABLE = {
    "p4_240x135": ((0, 6328, 11313, 15176, 18003, 20857), (3657, 2477, 1266, 1296, 1282)),
    "p13_200x150": ((0, 4164, 7015, 8955, 10003, 11096), (1934, 1148, 412, 431, 393)),
    "p5_200x150": ((0, 6338, 9857, 12337, 13706, 15131), (4534, 1850, 865, 669, 656)),
    "p7_200x150": ((0, 23254, 33757, 41568, 44957, 46533), (19624, 6138, 4333, 1656, 869)),
    "mtl_160x120": ((0, 12497, 34702, 65612, 118060, 231400), (2808, 1815, 2305, 1157, 1153)),
    "teapot2_240x135": ((0, 448, 825, 978, 979, 980), (61, 148, 0, 0, 0)),
}
DEPTH_TAGS = list(TABLE)
# the fixtures the reference harness wrote, recipe W: tag -> depths
FIXTURES = {"p4_240x135": (0, 1, 2, 3, 4), "mtl_160x120": (0, 1, 2, 3, 4), "p7_200x150": (1, 3), "p13_200x150": (2, 4),
            "teapot2_240x135": (1, 3)}
SAMPLED_FIXTURE = ("p10_s4_160x120", 2)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def bounce_fixture(tag, k):
    return np.load(os.path.join(GOLDEN, tag, "bounce%d.npz" % k))


@pytest.fixture(scope="module")
def depths(pkg, orc, golden):
    """(image, stats) of recipe W at depth k through the hook, rendered once per (tag, k) and never written to."""
    cache = {}

    def get(tag, k):
        if (tag, k) not in cache:
            g = golden(tag)
            out, st = orc.render(g.scene(pkg), g.width, g.height, threads=4, max_bounce=k)
            out.setflags(write=False)
            cache[(tag, k)] = (out, st)
        return cache[(tag, k)]
    return get


def test_the_fixtures_on_disk_are_the_ones_listed():
    found = {}
    for path in glob.glob(os.path.join(GOLDEN, "*", "bounce*.npz")):
        tag = os.path.basename(os.path.dirname(path))
        found.setdefault(tag, []).append(int(re.fullmatch(r"bounce(\d)\.npz", os.path.basename(path)).group(1)))
        assert os.path.getsize(path) <= os.path.getsize(os.path.join(GOLDEN, tag, "golden.npz")), path
    want = dict(FIXTURES)
    want[SAMPLED_FIXTURE[0]] = (SAMPLED_FIXTURE[1],)
    assert {t: tuple(sorted(v)) for t, v in found.items()} == want


@pytest.mark.parametrize("tag,k", [(t, k) for t, ks in FIXTURES.items() for k in ks])
def test_oracle_bit_exact_vs_reference_at_depth(orc, golden, depths, tag, k):
    """The comparison test_oracle.py makes with the depth-5 golden.npz of the same tag, at depth k."""
    g, f = golden(tag), bounce_fixture(tag, k)
    out, st = depths(tag, k)
    assert np.array_equal(bits(out[..., 3]), bits(f["z"])), "z differs"
    assert np.array_equal(bits(out[..., :3]), bits(f["rgb"])), "linear RGB differs"
    assert st["primary_rays"] == g.meta["primary"]
    assert st["primary_hits"] == int(f["primary_hits"]) == g.meta["primary_hits"]
    assert st["secondary_rays"] == int(f["secondary"])
    assert st["shadow_rays"] == int(f["shadow"])
    # z does not depend on the depth; gamma + Color24 + z-image as the reference's RenderImage holds them
    assert np.array_equal(bits(f["z"]), bits(g.npz["z"]))
    rgb8, _, zimg = orc.postprocess(out)
    assert np.array_equal(rgb8, f["result_u8"]) and np.array_equal(zimg, f["zbuffer_u8"])


def test_oracle_recipe_s_bit_exact_vs_reference_at_depth_2(pkg, orc, golden):
    tag, k = SAMPLED_FIXTURE
    g, f = golden(tag), bounce_fixture(tag, k)
    out, st = orc.render_samples(g.scene(pkg), g.width, g.height, g.meta["spp"], stream=orc.STREAM_SEQUENTIAL, trig=orc.TRIG_LIBM,
                                 threads=4, max_bounce=k)
    assert np.array_equal(bits(out[..., 3]), bits(f["z"])), "z differs"
    assert np.array_equal(bits(out[..., :3]), bits(f["rgb"])), "linear RGB differs"
    assert (st["primary_rays"], st["primary_hits"], st["secondary_rays"], st["shadow_rays"]) == (
        g.meta["primary"], int(f["primary_hits"]), int(f["secondary"]), int(f["shadow"]))
    rgb8, _, zimg = orc.postprocess(out)
    assert np.array_equal(rgb8, f["result_u8"]) and np.array_equal(zimg, f["zbuffer_u8"])
    # and the fixture is not the depth-5 one under another name
    assert int(f["secondary"]) < g.meta["secondary"] and not same_bits(f["rgb"], g.npz["rgb"])


def test_depth_5_through_the_hook_is_the_call_without_it(pkg, orc, golden):
    g = golden("p4_240x135")
    scene = g.scene(pkg)
    a, sa = orc.render(scene, g.width, g.height, threads=4)
    b, sb = orc.render(scene, g.width, g.height, threads=4, max_bounce=5)
    assert same_bits(a, b) and sa == sb and sa["secondary_rays"] == g.meta["secondary"]
    g = golden("p10_s4_160x120")
    scene = g.scene(pkg)
    for kw in (dict(stream=orc.STREAM_SEQUENTIAL, trig=orc.TRIG_LIBM), dict()):
        a, sa = orc.render_samples(scene, g.width, g.height, 2, threads=4, **kw)
        b, sb = orc.render_samples(scene, g.width, g.height, 2, threads=4, max_bounce=5, **kw)
        assert same_bits(a, b) and sa == sb
    g = golden("p13_p2_96x72")
    scene = g.scene(pkg)
    a, sa = orc.render_paths(scene, g.width, g.height, 2, threads=4)
    b, sb = orc.render_paths(scene, g.width, g.height, 2, threads=4, max_bounce=5)
    assert same_bits(a, b) and sa == sb
    assert same_bits(orc.sample_images(scene, g.width, g.height, 2, 0, 2, gi=True, threads=4),
                     orc.sample_images(scene, g.width, g.height, 2, 0, 2, gi=True, threads=4, max_bounce=5))
    a = orc.render_adaptive(scene, g.width, g.height, 4, 2, 1, 1e-3, gi=True, threads=4)
    b = orc.render_adaptive(scene, g.width, g.height, 4, 2, 1, 1e-3, gi=True, threads=4, max_bounce=5)
    assert same_bits(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[3] == b[3]


def test_no_call_leaves_the_oracle_at_another_depth(pkg, orc, golden):
    g = golden("teapot2_240x135")
    scene = g.scene(pkg)
    assert orc.max_bounce_now() == 5
    orc.render(scene, 32, 18, max_bounce=1)
    orc.render_samples(scene, 32, 18, 1, max_bounce=2)
    orc.render_paths(scene, 32, 18, 1, max_bounce=3)
    orc.sample_images(scene, 32, 18, 1, 0, 1, max_bounce=0)
    orc.render_adaptive(scene, 32, 18, 2, 1, 1, 0.0, max_bounce=4)
    assert orc.max_bounce_now() == 5
    with pytest.raises(orc.OracleError):  # a failing call restores it too
        orc.render(scene, 0, 0, max_bounce=2)
    assert orc.max_bounce_now() == 5
    for bad in (-1, 6):
        with pytest.raises(ValueError):
            orc.render(scene, 32, 18, max_bounce=bad)
    assert orc.max_bounce_now() == 5
    # the C hook: out-of-range values change nothing, the return value is the depth before the call
    assert orc.lib.rtu_oracle_debug_max_bounce(3) == 5 and orc.lib.rtu_oracle_debug_max_bounce(9) == 3
    assert orc.lib.rtu_oracle_debug_max_bounce(5) == 3 and orc.max_bounce_now() == 5


@pytest.mark.parametrize("tag", ["p4_240x135", "p7_200x150", "mtl_160x120"])
def test_depth_0_is_the_scene_without_mirrors_and_glass(pkg, orc, golden, depths, tag):
    """Shade() at bounceCount 0 is its light loop and nothing else, and so is Shade() of a material that neither reflects nor
    refracts at any depth: the second render does not go through the hook."""
    from test_gpu_scene_update import materials
    g = golden(tag)
    scene = g.scene(pkg)
    m = materials(scene)
    had = 0
    for i in range(scene.desc.n_materials):
        for c in range(3):
            had += (m[i].reflection[c] != 0) + (m[i].refraction[c] != 0)
            m[i].reflection[c] = 0.0
            m[i].refraction[c] = 0.0
    assert had, "nothing to take out: the scene has no recursive material"
    plain, sp = orc.render(scene, g.width, g.height, threads=4)
    zero, sz = depths(tag, 0)
    assert sp["secondary_rays"] == 0
    assert same_bits(plain, zero) and sp == sz


@pytest.mark.parametrize("tag", DEPTH_TAGS)
def test_every_depth_shows_as_the_table_says(golden, depths, tag):
    g = golden(tag)
    secondary, differing = TABLE[tag]
    assert secondary[5] == g.meta["secondary"], "the table's depth-5 entry is not the reference's counter"
    imgs = [depths(tag, k) for k in range(6)]
    assert tuple(st["secondary_rays"] for _, st in imgs) == secondary
    assert imgs[5][1]["shadow_rays"] == g.meta["shadow"]
    assert same_bits(imgs[5][0][..., :3], g.npz["rgb"])
    got = tuple(int((bits(imgs[k][0][..., :3]) != bits(imgs[k - 1][0][..., :3])).any(-1).sum()) for k in range(1, 6))
    assert got == differing
    for k in range(1, 6):
        assert same_bits(imgs[k][0][..., 3], imgs[0][0][..., 3]), "z depends on the depth"
        assert imgs[k][1]["shadow_rays"] >= imgs[k - 1][1]["shadow_rays"]


def test_oracle_vs_live_reference_build_at_depth_2(pkg, orc, golden, scene_files, tmp_path):
    """As test_oracle.py's test_oracle_vs_live_reference_build: where the reference harness of this tree is built, it renders the
    stored Project5 scene files at 176x132 with --bounces 2, and the oracle at depth 2 reproduces every bit and both counters.
    A ref_render that does not write the depth it rendered at into stats.json was built from an earlier driver.cpp, which takes no
    --bounces and renders at 5 whatever it is given: this tree's harness is then not built, and the test ends as it does without one."""
    import gzip
    import json
    import subprocess
    from conftest import MAC_PREFIX, REPO
    g = golden("p5_176x132")
    W, H = g.width, g.height
    out, st = orc.render(g.scene(pkg), W, H, threads=4, max_bounce=2)
    full, _ = orc.render(g.scene(pkg), W, H, threads=4)
    assert same_bits(full[..., :3], g.npz["rgb"]) and not same_bits(out[..., :3], full[..., :3])
    exe = os.path.join(REPO, "oracle", "_ref", "ref_render")
    if not os.path.exists(exe):
        return
    xml = tmp_path / "scene.xml"
    src = open(os.path.join(scene_files, "SceneFiles", "Project5", "scene.xml")).read()
    xml.write_text(src.replace(MAC_PREFIX, scene_files))
    subprocess.check_call([exe, str(xml), str(W), str(H), str(tmp_path), "4", "--bounces", "2"], stdout=subprocess.DEVNULL)
    stats = json.load(open(tmp_path / "stats.json"))
    if "bounces" not in stats:
        return
    assert stats["bounces"] == 2
    assert (tmp_path / "scene.rtus").read_bytes() == gzip.open(os.path.join(g.dir, "scene.rtus.gz")).read()
    z = np.fromfile(tmp_path / "z.f32", np.float32).reshape(H, W)
    rgb = np.fromfile(tmp_path / "rgb.f32", np.float32).reshape(H, W, 3)
    assert np.array_equal(bits(z), bits(out[..., 3])), "z differs"
    differ = (bits(rgb) != bits(out[..., :3])).any(-1)
    assert not differ.any(), "linear RGB differs at %d pixels (first %s; the live image %s the oracle's depth-5 image); live counters %s, oracle %s" % (
        int(differ.sum()), np.argwhere(differ)[0], "is" if same_bits(rgb, full[..., :3]) else "is not",
        (stats["secondary"], stats["shadow"]), (st["secondary_rays"], st["shadow_rays"]))
    assert (stats["primary_hits"], stats["secondary"], stats["shadow"]) == (st["primary_hits"], st["secondary_rays"], st["shadow_rays"])
