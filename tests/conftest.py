import json
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, "tests", "golden")
MAC_PREFIX = "/Users/Peter/GitRepos/RayTracer-Utah"  # the directory the reference's scene files name their meshes and textures by

SMALL_TAGS = ["p1_256", "p4_240x135", "teapot2_240x135", "p11_240x135"]
FULL_TAGS = ["p3s_800x600", "p4_1080", "teapot2_1080", "p11_1080"]
EXTRA_TAGS = ["p1test_200x150", "p2_200x150", "p3box_200x150", "p5_200x150", "p5low_200x150", "p11simple_200x150",
              "p13_200x150"]  # the reference's other deterministic scenes
SMALL_TAGS = SMALL_TAGS + EXTRA_TAGS
ALL_TAGS = SMALL_TAGS + FULL_TAGS
TEX_TAGS = ["p7_200x150", "mtl_160x120"]  # textured; mtl: an .obj with its own .mtl materials -> MultiMtl (row f3)
LOCAL_SCENES = {"mtl_160x120": "multimtl/scene.xml"}  # scenes written for this repository (tests/scenes), not the reference's


def instantiate_scene(rel, dst):
    """Copy tests/scenes/<dir of rel> to dst with its @DIR@ placeholders (absolute paths of .obj / texture files,
    as the reference's scene files carry them) pointing at dst; returns the path of the scene XML."""
    src = os.path.join(REPO, "tests", "scenes", os.path.dirname(rel))
    os.makedirs(str(dst), exist_ok=True)
    for name in os.listdir(src):
        data = open(os.path.join(src, name), "rb").read()
        if name.endswith((".xml", ".mtl", ".obj")):
            data = data.replace(b"@DIR@", str(dst).encode())
        open(os.path.join(str(dst), name), "wb").write(data)
    return os.path.join(str(dst), os.path.basename(rel))


def write_png_rgb(path, rgb, filters):
    """8-bit RGB PNG of rgb ([h, w, 3] uint8) with filters[y] (0-4) as the filter type of row y: with the filter types of
    an existing file this reproduces that file's filtered byte stream exactly (only the deflate layer can differ)."""
    import struct
    import zlib
    h, w, _ = rgb.shape
    x = rgb.reshape(h, w * 3).astype(np.int32)
    a = np.zeros_like(x)
    a[:, 3:] = x[:, :-3]   # the byte one pixel to the left
    b = np.zeros_like(x)
    b[1:] = x[:-1]         # the byte above
    c = np.zeros_like(x)
    c[1:] = a[:-1]         # above and to the left
    pa, pb, pc = np.abs(b - c), np.abs(a - c), np.abs(a + b - 2 * c)
    paeth = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))
    pred = [np.zeros_like(x), a, b, (a + b) >> 1, paeth]
    f = np.asarray(filters, np.int32)
    rows = np.take_along_axis(np.stack(pred), f[None, :, None].repeat(w * 3, axis=2), axis=0)[0]
    body = np.concatenate([f[:, None], (x - rows) & 255], axis=1).astype(np.uint8).tobytes()

    def chunk(typ, data):
        return struct.pack(">I", len(data)) + typ + data + struct.pack(">I", zlib.crc32(typ + data) & 0xFFFFFFFF)
    with open(path, "wb") as out:
        out.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0)) +
                  chunk(b"IDAT", zlib.compress(body, 9)) + chunk(b"IEND", b""))


def texture_pixels(pkg, scene, i):
    """Texture i of a loaded scene as [h, w, 3] uint8 (RtuTexture, include/rtu_scene.h); None without pixels."""
    import ctypes

    class Tex(ctypes.Structure):
        _fields_ = [("type", ctypes.c_int32), ("width", ctypes.c_int32), ("height", ctypes.c_int32), ("reserved", ctypes.c_int32),
                    ("rgb", ctypes.c_void_p), ("color1", ctypes.c_float * 3), ("color2", ctypes.c_float * 3)]
    t = Tex.from_address(scene.desc.textures + i * ctypes.sizeof(Tex))
    if not t.rgb:  # a checker, or a file that failed to load
        return None
    return np.ctypeslib.as_array((ctypes.c_uint8 * (t.width * t.height * 3)).from_address(t.rgb)).reshape(t.height, t.width, 3).copy()


@pytest.fixture(scope="session")
def scene_files(tmp_path_factory, pkg):
    """The reference's scene files (tests/golden/SceneFiles, written by make_goldens.py SceneFiles) as a tree
    <root>/SceneFiles/..., .obj files unpacked: load them with Scene.from_xml(path, MAC_PREFIX, <root>).
    The PNG textures are too large to store: each is written back from the pixels the reference decoded from it
    (a texture of a golden scene blob) with the filter type of every row of the original file (textures.json)."""
    import gzip
    import shutil
    root = tmp_path_factory.mktemp("reference")
    src = os.path.join(GOLDEN, "SceneFiles")
    for d, _, names in os.walk(src):
        out = os.path.join(str(root), "SceneFiles", os.path.relpath(d, src))
        os.makedirs(out, exist_ok=True)
        for name in names:
            if name.endswith(".gz"):
                with gzip.open(os.path.join(d, name), "rb") as f, open(os.path.join(out, name[:-3]), "wb") as g:
                    shutil.copyfileobj(f, g)
            elif name != "textures.json":
                shutil.copyfile(os.path.join(d, name), os.path.join(out, name))
    for rel, t in json.load(open(os.path.join(src, "textures.json"))).items():
        scene = pkg.Scene.from_blob_file(os.path.join(GOLDEN, t["tag"], "scene.rtus.gz"))
        write_png_rgb(os.path.join(str(root), "SceneFiles", rel), texture_pixels(pkg, scene, t["texture"]), [int(v) for v in t["filters"]])
    return str(root)


# stochastic effects, recipe S: glossy + soft + textured; depth of field; glossy + soft; 12 soft lights + glossy refraction; teapot + soft;
# glossy under a hard light (Project11/scene_glossy.xml: with it every scene file of the reference has a fixture)
SAMPLED_TAGS = ["p10_s4_160x120", "p9_s3_160x120", "p11gs_s2_160x90", "p11x86_s1_120x90", "teapot1_s2_160x90", "p11g_s2_160x90"]
PATH_TAGS = ["p11_p2_120x68", "p13_p2_96x72"]  # recipe P (config 5): + the Monte-Carlo gather


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def pkg():
    import __graft_entry__ as g
    return g.load_package()


@pytest.fixture(scope="session")
def orc():
    import __graft_entry__ as g
    return g.load_oracle()


class Golden:
    def __init__(self, tag):
        self.tag = tag
        self.dir = os.path.join(GOLDEN, tag)
        self.meta = json.load(open(os.path.join(self.dir, "meta.json")))
        self.width, self.height = self.meta["width"], self.meta["height"]
        self._npz = None

    @property
    def npz(self):
        if self._npz is None:
            self._npz = np.load(os.path.join(self.dir, "golden.npz"))
        return self._npz

    def scene(self, pkg):
        return pkg.Scene.from_blob_file(os.path.join(self.dir, "scene.rtus.gz"))


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def get(tag):
        if tag not in cache:
            cache[tag] = Golden(tag)
        return cache[tag]
    return get


def sha256(a):
    import hashlib
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def read_png(path):
    """Decode an 8-bit PNG with a tiny zlib-based reader (grey / RGB / palette / grey+alpha
    / RGBA, bit depths 1-8, non-interlaced) — enough for lodepng's auto-converted output."""
    import struct
    import zlib
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, idat, plte = 8, b"", None
    while pos < len(data):
        n, typ = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        pos += 12 + n
        if typ == b"IHDR":
            w, h, depth, ctype, _, _, interlace = struct.unpack(">IIBBBBB", body)
        elif typ == b"PLTE":
            plte = np.frombuffer(body, np.uint8).reshape(-1, 3)
        elif typ == b"IDAT":
            idat += body
    assert interlace == 0
    chans = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[ctype]
    bpp_bits = chans * depth
    stride = (w * bpp_bits + 7) // 8
    bpp = max(1, bpp_bits // 8)
    raw = zlib.decompress(idat)
    out = np.zeros((h, stride), np.uint8)
    prev = np.zeros(stride, np.int32)
    p = 0
    for y in range(h):
        ft = raw[p]
        line = np.frombuffer(raw, np.uint8, stride, p + 1).astype(np.int32)
        p += 1 + stride
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + prev) & 255
        else:
            cur = np.zeros(stride, np.int32)
            for i in range(stride):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                if ft == 1:
                    pred = a
                elif ft == 3:
                    pred = (a + b) >> 1
                else:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    pred = a if (pa <= pb and pa <= pc) else (b if pb <= pc else c)
                cur[i] = (line[i] + pred) & 255
        out[y] = cur
        prev = cur
    if depth < 8:
        bits = np.unpackbits(out, axis=1)[:, :w * bpp_bits].reshape(h, w * chans, depth)
        vals = (bits * (1 << np.arange(depth - 1, -1, -1))).sum(axis=2).astype(np.uint8)
        if ctype == 0:
            vals = (vals.astype(np.uint32) * 255 // ((1 << depth) - 1)).astype(np.uint8)
        px = vals.reshape(h, w, chans)
    else:
        px = out.reshape(h, w, chans)
    if ctype == 3:
        return plte[px[..., 0]]
    if ctype == 0:
        return px[..., 0]
    if ctype == 4:
        return px[..., 0]
    if ctype == 6:
        return px[..., :3]
    return px
