#!/usr/bin/env python3
"""Generate the golden fixtures under tests/golden/ from the COMPILED REFERENCE.

Authoring container only (needs /root/reference and oracle/_ref/ref_render, built
by `make -C oracle`). For every BASELINE config it runs the reference's own
Trace/Shade functions through oracle/ref_harness/driver.cpp ("recipe W",
SURVEY.md §8c; "recipe S" for the scenes with stochastic effects) and stores DATA only:

  scene.rtus.gz   flattened scene (input), serialised from the reference's
                  in-memory scene graph after LoadScene()
  Result.png      written by the reference's RenderImage::SaveImage (lodepng)
  ZBuffer.png     written by RenderImage::SaveZImage after ComputeZBufferImage
  golden.npz      full float z + linear RGB for the small configs; for 1080p an
                  every-8th-pixel subsample (z, rgb) plus the 8-bit images
  meta.json       resolution, ray counters, sha256 of the full float z / rgb /
                  8-bit buffers

`make_goldens.py bounces` (or `bounces:<tag>`) writes <tag>/bounce<k>.npz for the depths of BOUNCES: the same scene through
the same binary with the root Shade() calls given bounceCount k instead of 5 (ref_render --bounces k). A fixture reuses the
tag's scene.rtus.gz and holds z, rgb (float32), the two 8-bit images and the counters primary_hits, secondary, shadow.

`make_goldens.py SceneFiles` copies the reference's scene files that the loader tests read (tests/test_host.py,
tests/test_oracle.py) to tests/golden/SceneFiles/: every scene XML and the meshes they name, .obj files gzipped;
for the PNG textures only the filter type of each row and which texture of a golden blob holds their pixels
(textures.json), from which the tests write them back. They are the inputs of the fixtures above, so the loader is checked without the reference tree.

`make_goldens.py ref_trees` writes ref_trees/<name>_<n|c>.rtus.gz: the awkward meshes of tests/test_ref_build_host.py
(reference_meshes()) flattened by ref_render --scene-only, with vn lines (`n`) and without them (`c`: the reference's ComputeNormals).
They are loaded only, never rendered by the reference, so they need no `vt` lines (next paragraph).

An .obj that goes through the reference needs `vt` lines and `v/vt/vn` faces: TriObj::IntersectRay reads the texture
coordinates of every accepted hit unconditionally (objFunctions.cpp:320) and crashes on a mesh without them. The oracle
and the device render such a mesh (uvw = 0); the reference cannot, so the scenes under tests/scenes carry `vt`.

No reference source text is copied; the fixtures are inputs and outputs.
"""
import gzip, hashlib, json, os, shutil, subprocess, sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
RUN = os.path.join(REPO, "oracle", "ref_harness", "run_ref.sh")

CONFIGS = [
    # tag, scene (relative to SceneFiles), W, H, keep full floats[, spp (0: recipe W)[, "P" for recipe P[, depths]]]
    # depths: recursion depths other than the reference's 5 (RtuFrameDesc.max_bounce) that get a bounce<k>.npz next to golden.npz.
    # Between them every depth 0..4 has a recipe W fixture on a plain and on a textured scene, and recipe S has one.
    ("p1_256", "Project1Example.xml", 256, 256, True),
    ("p3s_800x600", "Project3Simple.xml", 800, 600, True),
    ("p4_1080", "Project4.xml", 1920, 1080, False),
    ("teapot2_1080", "Teapot/scene2.xml", 1920, 1080, False),
    ("p11_1080", "Project11/scene.xml", 1920, 1080, False),
    # small versions of the 1080p configs so CPU-only tests stay fast
    ("p4_240x135", "Project4.xml", 240, 135, True, 0, None, (0, 1, 2, 3, 4)),
    ("teapot2_240x135", "Teapot/scene2.xml", 240, 135, True, 0, None, (1, 3)),
    ("p11_240x135", "Project11/scene.xml", 240, 135, True),
    # the reference's other deterministic, untextured scenes, as extra regression inputs
    ("p1test_200x150", "Project1Test.xml", 200, 150, True),
    ("p2_200x150", "Project2.xml", 200, 150, True),
    ("p3box_200x150", "Project3Box.xml", 200, 150, True),
    ("p5_200x150", "Project5/scene.xml", 200, 150, True),
    ("p5low_200x150", "Project5/scene-low.xml", 200, 150, True),
    ("p11simple_200x150", "Project11/scene_simple.xml", 200, 150, True),
    ("p13_200x150", "Project13/scene.xml", 200, 150, True, 0, None, (2, 4)),
    # a resolution no other fixture renders this scene at (tests/test_oracle.py test_oracle_vs_live_reference_build)
    ("p5_176x132", "Project5/scene.xml", 176, 132, True),
    # textures ("next" row f2): checkerboards, two 1024x1024 PNGs (mesh diffuse, background, environment)
    ("p7_200x150", "Project7/scene.xml", 200, 150, True, 0, None, (1, 3)),
    # stochastic effects ("next" row f1), recipe S: the 7th field is samples per pixel. The reference is built
    # with rand() wrapped to the sequential sample stream (oracle/ref_harness/Makefile), so these are
    # reproducible: glossy reflection + refraction + a size-5 light + textures; depth of field + textures;
    # glossy reflections + a size-5 light; twelve size-1 lights + glossy refraction; the teapot under a size-5 light
    ("p10_s4_160x120", "Project10/scene.xml", 160, 120, True, 4, None, (2,)),
    ("p9_s3_160x120", "Project9/scene.xml", 160, 120, True, 3),
    ("p11gs_s2_160x90", "Project11/scene_glossy_soft.xml", 160, 90, True, 2),
    ("p11x86_s1_120x90", "Project11/scene_86.xml", 120, 90, True, 1),
    ("teapot1_s2_160x90", "Teapot/scene.xml", 160, 90, True, 2),
    # the last scene file of the reference without a fixture (round 3): glossy reflections under a hard point light
    ("p11g_s2_160x90", "Project11/scene_glossy.xml", 160, 90, True, 2),
    # row f3: an .obj that brings its own materials (usemtl / .mtl -> MultiMtl, xmlload.cpp:199-243) — a scene written for
    # this repository (tests/scenes/multimtl, "@" = repository path), run through the compiled reference like the others
    ("mtl_160x120", "@tests/scenes/multimtl/scene.xml", 160, 120, True, 0, None, (0, 1, 2, 3, 4)),
    # exact ties by the thousand (tests/scenes/ties): a torus pressed flat, three coincident grids lying in a `plane` object under
    # both node orders — which of the triangles (or the plane) with bitwise-equal t wins is the reference's test order
    ("ties_160x120", "@tests/scenes/ties/scene.xml", 160, 120, True),
    # node transformations no scene file of the reference has (tests/scenes/transforms, written by tests/test_oracle_transforms.py):
    # mirrored (negative scales); stretched 1e2 and 1e3 within a node; chains that cancel (1e4 x 1e-4, seven nodes deep); scales of 0,
    # 1e-30 and 1e30, whose inverses are NaN or infinite
    ("xf_t1_96x64", "@tests/scenes/transforms/t1.xml", 96, 64, True),
    ("xf_t2_96x64", "@tests/scenes/transforms/t2.xml", 96, 64, True),
    ("xf_t3_96x64", "@tests/scenes/transforms/t3.xml", 96, 64, True),
    ("xf_t4_96x64", "@tests/scenes/transforms/t4.xml", 96, 64, True),
    # recipe P (config 5): recipe S plus the 4-bounce Monte-Carlo gather of Render(); 8th field "P"
    ("p11_p2_120x68", "Project11/scene.xml", 120, 68, True, 2, "P"),
    ("p13_p2_96x72", "Project13/scene.xml", 96, 72, True, 2, "P"),
]

# tag -> files of other scene directories that its scene names beside itself (run_ref.sh EXTRA_ASSETS): the file texture of the
# transform scenes is multimtl's
ASSETS = {"xf_t%d_96x64" % k: ["tests/scenes/multimtl/tiles.png"] for k in (1, 2, 3, 4)}

# tag -> the depths of its bounce<k>.npz fixtures (the 8th field of a config)
BOUNCES = {c[0]: c[7] for c in CONFIGS if len(c) > 7}


# the files the scene XMLs name (absolute macOS paths, remapped to the copy by the tests); Teapot/ink*.png do not exist
SCENE_ASSETS = ["Project5/teapot.obj", "Project5/teapot-low.obj", "Project5/plane.obj", "Project7/teapot.obj"]
# too large to store: rebuilt by the tests (conftest.scene_files) from the pixels of a golden blob's texture and the
# filter type of each row of the file, recorded in SceneFiles/textures.json
SCENE_TEXTURES = {"Project7/bricks.png": "p7_200x150", "Project7/clouds.png": "p7_200x150"}


def png_rows(path):
    """(inflated IDAT stream, filter type of every row) of an 8-bit RGB PNG."""
    import struct
    import zlib
    d, pos, idat = open(path, "rb").read(), 8, b""
    while pos < len(d):
        n, typ = struct.unpack(">I4s", d[pos:pos + 8])
        if typ == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", d[pos + 8:pos + 8 + n])
            assert (depth, ctype, interlace) == (8, 2, 0), path
        elif typ == b"IDAT":
            idat += d[pos + 8:pos + 8 + n]
        pos += 12 + n
    raw = zlib.decompress(idat)
    return raw, "".join(str(raw[y * (w * 3 + 1)]) for y in range(h))


def copy_scene_files():
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.dirname(HERE))
    import tempfile
    import __graft_entry__
    from conftest import read_png, texture_pixels, write_png_rgb
    pkg = __graft_entry__.load_package()
    src = os.path.join(os.environ.get("REF", "/root/reference"), "SceneFiles")
    dst = os.path.join(HERE, "SceneFiles")
    rels = sorted(os.path.relpath(os.path.join(d, f), src) for d, _, fs in os.walk(src) for f in fs if f.endswith(".xml"))
    for rel in rels + SCENE_ASSETS:
        os.makedirs(os.path.dirname(os.path.join(dst, rel)), exist_ok=True)
        if rel.endswith(".obj"):
            with open(os.path.join(src, rel), "rb") as f, gzip.GzipFile(os.path.join(dst, rel + ".gz"), "wb", mtime=0) as g:
                g.write(f.read())
        else:
            shutil.copyfile(os.path.join(src, rel), os.path.join(dst, rel))
    textures = {}
    for rel, tag in sorted(SCENE_TEXTURES.items()):
        raw, filters = png_rows(os.path.join(src, rel))
        scene = pkg.Scene.from_blob_file(os.path.join(HERE, tag, "scene.rtus.gz"))
        pixels = read_png(os.path.join(src, rel))
        i = [k for k in range(scene.desc.n_textures) if np.array_equal(texture_pixels(pkg, scene, k), pixels)][0]
        with tempfile.TemporaryDirectory() as tmp:  # what the tests will write must be the original's filtered stream
            write_png_rgb(os.path.join(tmp, "t.png"), texture_pixels(pkg, scene, i), [int(v) for v in filters])
            assert png_rows(os.path.join(tmp, "t.png"))[0] == raw, rel
        textures[rel] = {"tag": tag, "texture": i, "filters": filters}
    json.dump(textures, open(os.path.join(dst, "textures.json"), "w"), indent=1, sort_keys=True)
    print("SceneFiles", len(rels), "scene files,", len(SCENE_ASSETS), "meshes,", len(textures), "textures")


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def save_npz(path, arrays):
    """An .npz (numpy.load reads it like any other) whose members are LZMA-compressed instead of deflated: a bounce<k>.npz may
    not be larger than its tag's golden.npz, and one whose image equals the depth-5 image carries three counters more."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w") as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.save(buf, np.asarray(arrays[name], order="C"))
            small = len(buf.getvalue()) < 1024
            zf.writestr(zipfile.ZipInfo(name + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                        zipfile.ZIP_STORED if small else zipfile.ZIP_LZMA)


def make_bounces(only):
    """<tag>/bounce<k>.npz for BOUNCES (only: the tags asked for, empty = all)."""
    for cfg in CONFIGS:
        tag, scene, W, H = cfg[:4]
        spp = cfg[5] if len(cfg) > 5 else 0
        if tag not in BOUNCES or (only and tag not in only):
            continue
        assert not (len(cfg) > 6 and cfg[6] == "P"), "MonteCarlo()'s own Shade calls keep their 5: no recipe P fixture at another depth"
        scene_arg = os.path.join(REPO, scene[1:]) if scene.startswith("@") else scene
        dst = os.path.join(HERE, tag)
        blob = gzip.open(os.path.join(dst, "scene.rtus.gz")).read()
        for k in BOUNCES[tag]:
            run = "%s_bounce%d" % (tag, k)
            subprocess.check_call([RUN, scene_arg, str(W), str(H), run, "8"] + ([str(spp)] if spp else []), env=dict(os.environ, BOUNCES=str(k)))
            src = os.path.join(REPO, "oracle", "_ref", "out", run)
            assert open(os.path.join(src, "scene.rtus"), "rb").read() == blob, "the fixture's scene is not the tag's scene.rtus.gz"
            stats = json.load(open(os.path.join(src, "stats.json")))
            assert stats["bounces"] == k and stats["spp"] == spp
            arrays = {
                "z": np.fromfile(os.path.join(src, "z.f32"), np.float32).reshape(H, W),
                "rgb": np.fromfile(os.path.join(src, "rgb.f32"), np.float32).reshape(H, W, 3),
                "result_u8": np.fromfile(os.path.join(src, "result.u8"), np.uint8).reshape(H, W, 3),
                "zbuffer_u8": np.fromfile(os.path.join(src, "zbuffer.u8"), np.uint8).reshape(H, W),
            }
            for name in ("primary_hits", "secondary", "shadow"):
                arrays[name] = np.int64(stats[name])
            out = os.path.join(dst, "bounce%d.npz" % k)
            save_npz(out, arrays)
            size, limit = os.path.getsize(out), os.path.getsize(os.path.join(dst, "golden.npz"))
            assert size <= limit, "%s: %d bytes, golden.npz has %d" % (out, size, limit)
            print(run, stats["primary_hits"], stats["secondary"], stats["shadow"], size, "bytes")
            shutil.rmtree(src)


def make_ref_trees():
    """ref_trees/<name>_<n|c>.rtus.gz: the meshes of tests/test_ref_build_host.py reference_meshes() as the compiled reference loads them
    (ref_render --scene-only, 64 x 48) — its own cyBVHTriMesh tree, element order, bounds and, for the `c` files (an .obj without vn
    lines), its ComputeNormals. `n`: the .obj carries vn lines. The .obj and .xml are written as the tests write them."""
    import pathlib
    import tempfile
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.dirname(HERE))
    from test_ref_build_host import reference_meshes, write_obj_scene
    exe = os.path.join(REPO, "oracle", "_ref", "ref_render")
    dst = os.path.join(HERE, "ref_trees")
    os.makedirs(dst, exist_ok=True)
    total = 0
    for name, (v, f) in reference_meshes().items():
        for normals in (True, False):
            with tempfile.TemporaryDirectory() as tmp:
                xml = write_obj_scene(pathlib.Path(tmp), name, v, f, normals)
                subprocess.check_call([exe, str(xml), "64", "48", tmp, "1", "--scene-only"], stdout=subprocess.DEVNULL)
                out = os.path.join(dst, "%s_%s.rtus.gz" % (name, "n" if normals else "c"))
                with open(os.path.join(tmp, "scene.rtus"), "rb") as g, gzip.GzipFile(out, "wb", mtime=0) as z:
                    z.write(g.read())
            total += os.path.getsize(out)
            print(os.path.basename(out), os.path.getsize(out), "bytes")
    print("ref_trees", 2 * len(reference_meshes()), "blobs,", total, "bytes")


def main():
    only = set(sys.argv[1:])
    if "ref_trees" in only:
        make_ref_trees()
        only.discard("ref_trees")
        if not only:
            return
    bounce_tags = {a.split(":", 1)[1] for a in only if a.startswith("bounces:")}
    if "bounces" in only or bounce_tags:
        make_bounces(bounce_tags)
        only = {a for a in only if a != "bounces" and not a.startswith("bounces:")}
        if not only:
            return
    if "SceneFiles" in only:
        copy_scene_files()
        only.discard("SceneFiles")
        if not only:
            return
    for cfg in CONFIGS:
        tag, scene, W, H, full = cfg[:5]
        spp = cfg[5] if len(cfg) > 5 else 0
        paths = len(cfg) > 6 and cfg[6] == "P"
        if only and tag not in only:
            continue
        scene_arg = os.path.join(REPO, scene[1:]) if scene.startswith("@") else scene
        subprocess.check_call([RUN, scene_arg, str(W), str(H), tag, "8"] + ([str(spp)] if spp else []) + (["paths"] if paths else []),
                              env=dict(os.environ, EXTRA_ASSETS=" ".join(os.path.join(REPO, a) for a in ASSETS.get(tag, []))))
        src = os.path.join(REPO, "oracle", "_ref", "out", tag)
        dst = os.path.join(HERE, tag)
        os.makedirs(dst, exist_ok=True)
        with open(os.path.join(src, "scene.rtus"), "rb") as f, gzip.GzipFile(
            os.path.join(dst, "scene.rtus.gz"), "wb", mtime=0) as g:
            g.write(f.read())
        for png in ("Result.png", "ZBuffer.png"):
            shutil.copyfile(os.path.join(src, png), os.path.join(dst, png))
        z = np.fromfile(os.path.join(src, "z.f32"), np.float32).reshape(H, W)
        rgb = np.fromfile(os.path.join(src, "rgb.f32"), np.float32).reshape(H, W, 3)
        res8 = np.fromfile(os.path.join(src, "result.u8"), np.uint8).reshape(H, W, 3)
        z8 = np.fromfile(os.path.join(src, "zbuffer.u8"), np.uint8).reshape(H, W)
        stats = json.load(open(os.path.join(src, "stats.json")))
        meta = {
            "scene": scene, "width": W, "height": H, "recipe": "P" if paths else "S" if spp else "W", "spp": spp,
            "stream": "sequential" if spp else None,
            "primary": stats["primary"], "primary_hits": stats["primary_hits"],
            "secondary": stats["secondary"], "shadow": stats["shadow"],
            "sha256_z_f32": sha(z), "sha256_rgb_f32": sha(rgb),
            "sha256_result_u8": sha(res8), "sha256_zbuffer_u8": sha(z8),
            "sum_result_u8": int(res8.astype(np.uint64).sum()),
            "sum_zbuffer_u8": int(z8.astype(np.uint64).sum()),
            "nonzero_zbuffer_u8": int((z8 != 0).sum()),
        }
        arrays = {"result_u8": res8, "zbuffer_u8": z8}
        if full:
            arrays["z"] = z
            arrays["rgb"] = rgb
        else:
            arrays["z_sub8"] = z[::8, ::8].copy()
            arrays["rgb_sub8"] = rgb[::8, ::8].copy()
        np.savez_compressed(os.path.join(dst, "golden.npz"), **arrays)
        json.dump(meta, open(os.path.join(dst, "meta.json"), "w"), indent=1, sort_keys=True)
        print(tag, meta["primary_hits"], meta["secondary"], meta["shadow"])
        shutil.rmtree(src)  # the raw dumps are large (40 MB per 1080p config); the fixtures are what is kept


if __name__ == "__main__":
    sys.exit(main())
