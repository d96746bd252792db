"""Exact ties by construction (tests/scenes/ties, golden ties_160x120). No GPU.

A mesh that is flat in an object-space axis plane has the face normal (+-0, +-0, +-1) exactly (norm3 is a / sqrtf(dot)), so
t = dot(A - p, N) / dot(dir, N) has the same bits for every triangle of the mesh: any ray through two accepting triangles ties, and
the winner is the one the reference's walk tests first. A `plane` object beside such a mesh in one group sees the same object-space
ray and computes (-p.z) / dir.z: the same bits again, the winner is the earlier node.

  pancake.obj   a torus of 24 x 10 quads with every z = 0 (two layers over every point of the annulus), the normals of the round
                torus, faces shuffled;
  card.obj      three coincident 8 x 8 grids at z = 0 inside [-0.8, 0.8]^2, a tilted normal per layer, faces shuffled;
  scene.xml     the pancake; the card beside a `plane` under two groups, plane first in one, card first in the other; a mirror floor,
                a point and a direct light.

Both files carry `vt` lines: the reference cannot render a mesh without them (tests/golden/make_goldens.py).

Here: the oracle equals the compiled reference on this scene bit for bit, and the fixture is not vacuous — the face order alone
changes hundreds of pixels. The scene builders below are shared with test_gpu_ties.py."""
import math
import random

import numpy as np

from conftest import instantiate_scene

TAG = "ties_160x120"
PANCAKE_NU, PANCAKE_NV = 24, 10  # quads around / across the tube: vertex i * (NV + 1) + j


def ties_scene(pkg, dst, edits=(), name="scene.xml"):
    """tests/scenes/ties instantiated in dst, its XML with every (old, new) of `edits` applied, loaded."""
    import os
    xml = instantiate_scene("ties/scene.xml", dst)
    text = open(xml).read()
    for old, new in edits:
        assert old in text, old
        text = text.replace(old, new)
    path = os.path.join(str(dst), name)
    open(path, "w").write(text)
    return pkg.Scene.from_xml(path)


def mesh_of(scene, nv):
    """The index of the mesh with nv vertices (pancake: 275, card: 243)."""
    found = [m for m in range(scene.desc.n_meshes) if scene.mesh(m).nv == nv]
    assert len(found) == 1
    return found[0]


def pancake(scene):
    return mesh_of(scene, (PANCAKE_NU + 1) * (PANCAKE_NV + 1))


def round_vertices(v):
    """The pancake's vertices with the z of the round torus (tube radius 0.7) they were pressed flat from."""
    out = np.array(v, np.float32)
    j = np.arange(len(out)) % (PANCAKE_NV + 1)
    out[:, 2] = (0.7 * np.sin(2 * math.pi * j / PANCAKE_NV)).astype(np.float32)
    return out


def welded_vertices(v):
    """The pancake's vertices with x > 0 all moved to one point: zero-area triangles (NaN records) among tying ones."""
    out = np.array(v, np.float32)
    out[out[:, 0] > 0] = (1.0, 0.5, 0.0)
    return out


def with_vertices(pkg, scene, mesh, v):
    out = pkg.Scene(pkg.host.rtu_scene_clone(scene.desc_ptr))
    out.set_mesh_vertices(mesh, v)
    return out


def shuffle_faces(path, seed):
    """The .obj at `path` with its `f` lines in another order (nothing else moves)."""
    lines = open(path).read().split("\n")
    at = [i for i, line in enumerate(lines) if line.startswith("f ")]
    faces = [lines[i] for i in at]
    random.Random(seed).shuffle(faces)
    for i, line in zip(at, faces):
        lines[i] = line
    open(path, "w").write("\n".join(lines))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_oracle_equals_the_reference_on_exact_ties(pkg, orc, golden, tmp_path):
    """z, linear RGB and the ray counters of the compiled reference, bit for bit: the oracle's tie order is the reference's. The
    scene files under tests/scenes/ties are the golden's scene."""
    g = golden(TAG)
    for scene in (g.scene(pkg), ties_scene(pkg, tmp_path)):
        out, st = orc.render(scene, g.width, g.height, threads=4)
        assert same_bits(out[..., 3], g.npz["z"]), "z differs"
        assert same_bits(out[..., :3], g.npz["rgb"]), "linear RGB differs"
        assert (st["primary_rays"], st["primary_hits"], st["secondary_rays"], st["shadow_rays"]) == (
            g.meta["primary"], g.meta["primary_hits"], g.meta["secondary"], g.meta["shadow"])


def test_the_face_order_shows_in_the_image(pkg, orc, golden, tmp_path):
    """The fixture is not vacuous: with the faces of both meshes in another order the same surfaces are hit at the same t (z bit-
    identical), and another triangle wins at hundreds of pixels. At least 200 is a condition on the fixture (this one: 803 of
    19200), not a tolerance."""
    g = golden(TAG)
    a, _ = orc.render(ties_scene(pkg, tmp_path), g.width, g.height, threads=4)
    shuffle_faces(str(tmp_path / "pancake.obj"), 1)
    shuffle_faces(str(tmp_path / "card.obj"), 2)
    b, _ = orc.render(pkg.Scene.from_xml(str(tmp_path / "scene.xml")), g.width, g.height, threads=4)
    assert same_bits(a[..., 3], b[..., 3]), "the face order moved a surface"
    changed = int((a[..., :3] != b[..., :3]).any(axis=2).sum())
    print("the face order changes the colour of %d pixels" % changed)
    assert changed >= 200


def test_the_two_node_orders_show_different_winners(pkg, orc, golden):
    """The card lies in a `plane` object under two groups. Left half of the image: the card is the earlier node and wins (yellow
    inside a blue rim); right half: the plane is the earlier node and wins everywhere (no yellow pixel at all)."""
    g = golden(TAG)
    yellow, blue = card_and_plane_pixels(g.npz["rgb"])
    half = g.width // 2
    assert yellow[:, :half].sum() > 500 and yellow[:, half:].sum() == 0
    assert blue[:, half:].sum() > 1000 and blue[:, :half].sum() > 100


def card_and_plane_pixels(rgb):
    """Masks of the pixels that show the card's material (yellow) and the plane's (blue) in a linear RGB image."""
    r, gr, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    return (r > 2 * b) & (gr > 2 * b) & (r > 0.1), (b > 2 * r) & (b > 2 * gr) & (b > 0.1)
