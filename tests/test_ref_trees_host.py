"""The awkward meshes of test_ref_build_host.py (reference_meshes()) against trees the COMPILED REFERENCE built: tests/golden/ref_trees
holds, per mesh, the scene blob ref_render --scene-only flattened from the files write_obj_scene writes (make_goldens.py ref_trees) —
`n` from an .obj with vn lines, `c` from one without, where the reference ran its ComputeNormals. No GPU.

  * the loader on the regenerated files gives the fixture's bytes;
  * the host form of the device builder (rtu_debug_host_ref_build), on the fixture's connectivity and vertices, gives the fixture's tree
    renumbered breadth-first, its element order, node count, depth, mesh box, any_empty_box and — for the `c` fixtures — normals;
  * where the reference harness of this tree is built, it is run live and must write the stored bytes;
  * the fixtures hold what they are for: the deep row's 57 levels, single leaves of 5 to 8 inseparable triangles, both zeros, centres
    that overflow, subnormal boxes, NaN normals.

The fixtures and their helpers are defined here once (test_gpu_ref_trees.py imports them)."""
import gzip
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, REPO
from test_mesh_update_host import RTU_MAX_BVH_STACK, clone
from test_ref_build_host import assert_build_equals_host, host_tree, reference_meshes, vn_of, write_obj_scene

REF_TREES = os.path.join(GOLDEN, "ref_trees")
MESHES = reference_meshes()
KINDS = ("n", "c")  # the .obj carries vn lines / the reference computed the normals
FIXTURES = [(name, kind) for name in MESHES for kind in KINDS]
FIXTURE_IDS = ["%s_%s" % nk for nk in FIXTURES]
W, H = 64, 48


def fixture_path(name, kind):
    return os.path.join(REF_TREES, "%s_%s.rtus.gz" % (name, kind))


def fixture_bytes(name, kind):
    with gzip.open(fixture_path(name, kind)) as g:
        return g.read()


def fixture_scene(pkg, name, kind):
    """The scene the reference flattened: its mesh 0 holds the reference's own tree, element order, bounds and normals."""
    return pkg.Scene.from_blob_file(fixture_path(name, kind))


def other_vertices(nv, seed=4242):
    """nv vertices that are none of a fixture's: what a mesh holds before it takes the fixture's."""
    return (np.random.RandomState(seed).rand(nv, 3) * 4 - 2).astype(np.float32)


def stale_copy(pkg, scene):
    """A clone of `scene` whose mesh 0 has other vertices (and the tree, bounds and normals that go with them): only the connectivity
    is the fixture's."""
    base = clone(pkg, scene)
    base.set_mesh_vertices(0, other_vertices(scene.mesh(0).nv))
    assert base.to_blob_bytes() != scene.to_blob_bytes()
    return base


def test_every_fixture_file_is_a_mesh_of_the_list():
    assert len(MESHES) == 25 and len(FIXTURES) == 50
    assert sorted(os.listdir(REF_TREES)) == sorted(os.path.basename(fixture_path(*nk)) for nk in FIXTURES)


@pytest.mark.parametrize("name,kind", FIXTURES, ids=FIXTURE_IDS)
def test_loader_matches_the_reference(pkg, tmp_path, name, kind):
    v, f = MESHES[name]
    scene = pkg.Scene.from_xml(str(write_obj_scene(tmp_path, name, v, f, normals=kind == "n")))
    scene.set_resolution(W, H)
    want = fixture_bytes(name, kind)
    assert scene.to_blob_bytes() == want, "the loader's scene is not the one the reference flattened"
    F = fixture_scene(pkg, name, kind)
    assert F.to_blob_bytes() == want and F.desc.n_meshes == 1
    m = F.mesh(0)
    assert (m.nv, m.nf, m.nvn) == (len(v), len(f), len(v))
    assert np.array_equal(F.mesh_vertices(0).view(np.uint32), v.view(np.uint32)), "%.9g did not carry the vertices through the reference"


@pytest.mark.parametrize("name,kind", FIXTURES, ids=FIXTURE_IDS)
def test_host_form_matches_the_reference(pkg, name, kind):
    F = fixture_scene(pkg, name, kind)
    base = stale_copy(pkg, F)
    got = assert_build_equals_host(pkg, base, 0, F, "%s_%s" % (name, kind))
    if kind == "c":
        want = vn_of(F, 0)
        assert np.array_equal(got["vn"].view(np.uint32), want.view(np.uint32)), "normals differ from the reference's ComputeNormals at %d words" % int(
            (got["vn"].view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("name,kind", FIXTURES, ids=FIXTURE_IDS)
def test_live_reference_writes_the_fixture(tmp_path, name, kind):
    """Where the reference harness of this tree is built: it reproduces the stored blob from the regenerated files."""
    exe = os.path.join(REPO, "oracle", "_ref", "ref_render")
    if not os.path.exists(exe):
        return
    v, f = MESHES[name]
    xml = write_obj_scene(tmp_path, name, v, f, normals=kind == "n")
    subprocess.check_call([exe, str(xml), str(W), str(H), str(tmp_path), "1", "--scene-only"], stdout=subprocess.DEVNULL)
    assert (tmp_path / "scene.rtus").read_bytes() == fixture_bytes(name, kind)


# ---- what the fixtures hold ----------------------------------------------------------------------------------------------------------

def tree_words(scene):
    """[nodes, 8] uint32 {bmin, index, bmax, count} of mesh 0 as the reference numbered it (node 0 unused)."""
    m = scene.mesh(0)
    import ctypes
    return np.ctypeslib.as_array(ctypes.cast(m.bvh, ctypes.POINTER(ctypes.c_uint32)), (m.n_bvh_nodes, 8)).copy()


def box_words(scene):
    t = tree_words(scene)[1:]
    return np.concatenate([t[:, 0:3].reshape(-1), t[:, 4:7].reshape(-1)])


@pytest.mark.parametrize("kind", KINDS)
def test_what_the_fixtures_hold(pkg, kind):
    deep = fixture_scene(pkg, "deep60", kind).mesh(0)
    assert deep.bvh_depth == 57 > RTU_MAX_BVH_STACK and deep.n_bvh_nodes == 114
    assert fixture_scene(pkg, "deep40", kind).mesh(0).bvh_depth == 37
    for name in MESHES:
        if name != "deep60":  # the one fixture the device path must refuse
            assert fixture_scene(pkg, name, kind).mesh(0).bvh_depth <= RTU_MAX_BVH_STACK, name
    for n in range(5, 9):
        F = fixture_scene(pkg, "coincident%d" % n, kind)
        t = tree_words(F)
        assert F.mesh(0).n_bvh_nodes == 2 and F.mesh(0).bvh_depth == 1 and t[1, 7] == n and t[1, 3] == 0, "coincident%d is not one leaf" % n
    for n in (5, 8, 9):  # ... while separable soups of those sizes are split
        assert fixture_scene(pkg, "soup%d" % n, kind).mesh(0).n_bvh_nodes > 2
    b = box_words(fixture_scene(pkg, "signed_zero", kind))
    assert (b == 0x80000000).any() and (b == 0).any(), "signed_zero: the boxes hold only one of the zeros"
    v, f = MESHES["huge"]
    with np.errstate(over="ignore"):
        centres = ((v[f[:, 0]] + v[f[:, 1]]) + v[f[:, 2]]) / np.float32(3)
    assert np.isinf(centres).any() and np.isfinite(v).all(), "huge: no centre sum overflows"
    b = box_words(fixture_scene(pkg, "denormal", kind))
    assert (((b & 0x7F800000) == 0) & ((b & 0x007FFFFF) != 0)).any(), "denormal: no subnormal box word"
    for name, bad in (("nan", np.isnan), ("inf", np.isinf)):
        F = fixture_scene(pkg, name, kind)
        assert bad(F.mesh_vertices(0)[5, 1]) and int(bad(F.mesh_vertices(0)).sum()) == 1, name + ": the value did not come through the reference"
    t = tree_words(fixture_scene(pkg, "mean_on_centre", kind))
    root = t[1].view(np.float32)
    assert 0.5 * (root[0] + root[4]) == 0.0 and t[1, 7] == 0, "mean_on_centre: the middle of the root's box is not the middle triangle's centre"
    vn = vn_of(fixture_scene(pkg, "collapse", kind), 0)
    assert np.isnan(vn).any() == (kind == "c"), "collapse: NaN normals where the reference computed them, none where the file carries them"
    # the tree of a fixture, renumbered, is a tree: every element once, children after their parents
    for name in ("grid", "flat60", "flatten"):
        F = fixture_scene(pkg, name, kind)
        tree, el, _ = host_tree(F, 0)
        assert sorted(el) == list(range(F.mesh(0).nf))
        inner = tree[1:F.mesh(0).n_bvh_nodes][tree[1:F.mesh(0).n_bvh_nodes, 7] == 0]
        assert len(inner) and np.all(inner[:, 3] > 1)
