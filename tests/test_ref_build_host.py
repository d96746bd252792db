"""The reference's mean-split tree restated level by level (csrc/rtu_ref_build.h), in its HOST FORM: the same passes the GPU runs for
rtu_update_meshes_device, run in loops (rtu_debug_host_ref_build, rtu_debug_partition_rule). No GPU.

  * the closed form of partition_from_back against a transcription of the loop;
  * tree, element order, depth, node count, mesh box and any_empty_box against rtu_scene_set_mesh_vertices + renumber_bfs, bit for bit;
  * normals by vertex adjacency against ComputeNormals.

The small meshes are defined here once (test_gpu_mesh_update_device.py imports them), and so are the meshes of tests/golden/ref_trees
(reference_meshes(); test_ref_trees_host.py and test_gpu_ref_trees.py hold them to trees the compiled reference built)."""
import ctypes
import itertools

import numpy as np
import pytest

from test_mesh_update_host import DEFORMATIONS, RTU_MAX_BVH_STACK, clone, deform_name, deformed_scene, deformed_vertices

XML = """<xml><scene>
  <object type="obj" name="{o}" material="m"><translate x="0.5" z="1"/></object>
  <object type="plane" name="floor" material="m"><scale value="30"/><translate z="-4"/></object>
  <material type="blinn" name="m"><diffuse r="0.6" g="0.6" b="0.6"/></material>
  <light type="point" name="p"><intensity value="0.7"/><position x="10" y="-20" z="30"/></light>
</scene><camera><position x="0" y="-12" z="4"/><target x="0" y="0" z="0"/><up x="0" y="0" z="1"/><fov value="45"/>
  <width value="64"/><height value="48"/></camera></xml>"""


def write_obj_scene(dst, name, v, f, normals=True):
    """The files of a scene of one mesh: vertices v [nv, 3], faces f [nf, 3] (0-based); normals: the file carries one vn per vertex
    (else the loader computes them: ComputeNormals). Returns the path of the scene XML."""
    dst.mkdir(parents=True, exist_ok=True)
    obj = dst / (name + ".obj")
    with open(str(obj), "w") as g:
        for p in v:
            g.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in p))
        if normals:
            for _ in v:
                g.write("vn 0 0 1\n")
        for t in f:
            g.write("f " + " ".join(("%d//%d" % (i + 1, i + 1)) if normals else str(i + 1) for i in t) + "\n")
    xml = dst / (name + ".xml")
    xml.write_text(XML.format(o=obj))
    return xml


def obj_scene(pkg, dst, name, v, f, normals=True):
    """write_obj_scene's files, loaded."""
    return pkg.Scene.from_xml(str(write_obj_scene(dst, name, v, f, normals)))


def soup(n, seed):
    """n random triangles, no shared vertex."""
    rng = np.random.RandomState(seed)
    v = (rng.rand(3 * n, 3) * 4 - 2).astype(np.float32)
    return v, np.arange(3 * n).reshape(n, 3)


def coincident(n):
    """n copies of one triangle: no axis separates them."""
    v = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0.5]], np.float32)
    return v, np.tile(np.arange(3), (n, 1))


def deep_row(n=60, ratio=0.5):
    """n small triangles whose centres sit at ratio^k: every split takes one off the far end (depth 57 for 60 at 0.5)."""
    v = []
    for k in range(n):
        c = np.float32(ratio) ** np.float32(k)
        e = c * np.float32(0.01)
        v += [[c - e, 0, 0], [c + e, e, 0], [c, 0, e]]
    return np.array(v, np.float32), np.arange(3 * n).reshape(n, 3)


def flat_row(n=60):
    """The connectivity of deep_row with centres at k: a shallow tree."""
    v = []
    for k in range(n):
        v += [[k - 0.3, 0, 0], [k + 0.3, 0.3, 0], [k, 0, 0.3]]
    return np.array(v, np.float32), np.arange(3 * n).reshape(n, 3)


def small_meshes():
    """name -> (v, f): the soups around the leaf limits 4 and 8."""
    out = {}
    for n in range(1, 10):
        out["soup%d" % n] = soup(n, n)
    for n in range(5, 9):
        out["coincident%d" % n] = coincident(n)
    return out


def mean_on_centre():
    """Nine triangles with centres at k = -4 ... 4 on x: the mean of the centres, 0, is exactly the middle one's."""
    v = []
    for k in range(-4, 5):
        v += [[k - 0.25, 0, 0], [k + 0.25, 0, 0], [k, 0.5, 0]]
    return np.array(v, np.float32), np.arange(27).reshape(9, 3)


def grid(n=12):
    """An n x n lattice of vertices at integer (x, y, 0), each quad split in two: 2 (n - 1)^2 faces with many equal centre coordinates."""
    v = np.array([[x, y, 0] for y in range(n) for x in range(n)], np.float32)
    f = []
    for y in range(n - 1):
        for x in range(n - 1):
            a = y * n + x
            f += [[a, a + 1, a + n], [a + 1, a + n + 1, a + n]]
    return v, np.array(f)


def reference_meshes():
    """name -> (v, f): the meshes whose trees tests/golden/ref_trees holds as the compiled reference built them (make_goldens.py
    ref_trees): the small meshes, rows that peel one element per level, degenerate meshes and coordinates at the edges of binary32."""
    out = dict(small_meshes())
    out["deep60"] = deep_row()
    out["deep40"] = deep_row(40)
    out["flat60"] = flat_row()
    v, f = soup(40, 7)
    out["collapse"] = (np.full_like(v, 1.25), f)
    flat = v.copy()
    flat[:, 2] = 0
    out["flatten"] = (flat, f)
    z = v.copy()
    z[1::2, 0], z[0::2, 0] = 0.0, -0.0
    out["signed_zero"] = (z, f)
    with np.errstate(over="ignore"):
        out["huge"] = (v * np.float32(1e38), f)
    out["denormal"] = (v * np.float32(1e-40), f)
    out["mean_on_centre"] = mean_on_centre()
    for name, x in (("nan", np.nan), ("inf", np.inf)):
        w = v.copy()
        w[5, 1] = x
        out[name] = (w, f)
    out["grid"] = grid()
    for v, _ in out.values():
        assert v.dtype == np.float32
    return out


def nan_variants(v):
    """The vertices v with one NaN in the middle / with vertex 0 NaN."""
    a, b = np.array(v, np.float32), np.array(v, np.float32)
    a[len(a) // 2, 1] = np.nan
    b[0] = np.nan
    return {"one NaN vertex": a, "v[0] NaN": b}


def host_tree(scene, mesh):
    """ref_bvh [nodes, 8] uint32 — the mesh's tree renumbered breadth-first (renumber_bfs restated) —, elements, any_empty_box."""
    m = scene.mesh(mesh)
    t = np.ctypeslib.as_array(ctypes.cast(m.bvh, ctypes.POINTER(ctypes.c_uint32)), (m.n_bvh_nodes, 8)).copy()
    el = np.ctypeslib.as_array(ctypes.cast(m.elements, ctypes.POINTER(ctypes.c_uint32)), (m.n_elements,)).copy()
    f = t.view(np.float32)
    with np.errstate(invalid="ignore"):
        empty = int(bool((f[1:, 0:3] > f[1:, 4:7]).any()))
    out = np.zeros_like(t)
    queue, nxt, qi = [(1, 1)], 2, 0
    while qi < len(queue):
        old, new = queue[qi]
        qi += 1
        node = t[old].copy()
        if node[7] == 0:
            queue += [(int(node[3]), nxt), (int(node[3]) + 1, nxt + 1)]
            node[3] = nxt
            nxt += 2
        out[new] = node
    return out, el, empty


def assert_build_equals_host(pkg, uploaded, mesh, now, what):
    """The host form on the connectivity of `uploaded` with the vertices of `now` against the tree set_mesh_vertices left in `now`."""
    m = now.mesh(mesh)
    got = pkg.host_ref_build(uploaded, mesh, now.mesh_vertices(mesh))
    tree, el, empty = host_tree(now, mesh)
    print("%s: %d nodes, depth %d" % (what, m.n_bvh_nodes, m.bvh_depth))
    assert got["n_bvh_nodes"] == m.n_bvh_nodes and got["bvh_depth"] == m.bvh_depth, "%s: %d nodes, depth %d; host %d, %d" % (
        what, got["n_bvh_nodes"], got["bvh_depth"], m.n_bvh_nodes, m.bvh_depth)
    assert np.array_equal(got["ref_elements"], el), what + ": element order differs"
    assert np.array_equal(got["ref_bvh"], tree), "%s: tree differs at %d words" % (what, int((got["ref_bvh"] != tree).sum()))
    assert got["any_empty_box"] == empty, what + ": any_empty_box"
    for key, want in (("bmin", m.bound_min), ("bmax", m.bound_max)):
        assert np.array_equal(got[key].view(np.uint32), np.array(list(want), np.float32).view(np.uint32)), "%s: %s differs" % (what, key)
    if m.bvh_depth <= RTU_MAX_BVH_STACK:  # ... and against the restatement the device path's tests compare with
        ref = pkg.host_mesh(now, mesh)
        assert np.array_equal(got["ref_bvh"], ref["ref_bvh"]) and np.array_equal(got["ref_elements"], ref["ref_elements"])
        assert np.float32(got["scale"]).view(np.uint32) == np.float32(ref["scale"]).view(np.uint32) and got["any_empty_box"] == ref["any_empty_box"]
    return got


# ---- 1. the partition -------------------------------------------------------------------------------------------------------------

def partition_from_back(keep):
    """host/mesh.cpp's loop on the identity order: a[i] is the position whose element ends at i."""
    a = list(range(len(keep)))
    left, end = 0, len(keep)
    while left < end:
        if keep[a[left]]:
            left += 1
            continue
        end -= 1
        a[left], a[end] = a[end], a[left]
    return a


def test_partition_rule_every_mask_to_12(pkg):
    for n in range(0, 13):
        for keep in itertools.product((0, 1), repeat=n):
            assert list(pkg.partition_rule(keep)) == partition_from_back(keep), keep


def test_partition_rule_random_masks(pkg):
    rng = np.random.RandomState(7)
    sizes = [13, 64, 65, 255, 256, 257, 500, 1999, 2000]
    for n in sizes + [int(x) for x in rng.randint(13, 2001, 40)]:
        for p in (0.0, 1.0, 0.01, 0.99, 0.5, float(rng.rand())):
            keep = (rng.rand(n) < p).astype(np.uint8)
            assert list(pkg.partition_rule(keep)) == partition_from_back(list(keep)), (n, p)


# ---- 2. the tree ------------------------------------------------------------------------------------------------------------------

def check_deformations(pkg, scene, meshes, tag):
    depths = set()
    for mesh in meshes:
        assert_build_equals_host(pkg, scene, mesh, scene, "%s mesh %d as loaded" % (tag, mesh))
        for d in DEFORMATIONS:
            now = deformed_scene(pkg, scene, mesh, d)
            depths.add(now.mesh(mesh).bvh_depth)
            assert_build_equals_host(pkg, scene, mesh, now, "%s mesh %d %s" % (tag, mesh, deform_name(d)))
    return depths


def test_tree_teapot(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    assert scene.desc.n_meshes == 1 and scene.mesh(0).nf == 6320
    assert len(check_deformations(pkg, scene, [0], "teapot")) > 1


def test_tree_torus(pkg, tmp_path):
    from test_gpu_scene_update import torus_scene
    check_deformations(pkg, torus_scene(pkg, tmp_path), [0], "torus")


def test_tree_ties(pkg, tmp_path):
    from test_ties_host import ties_scene
    scene = ties_scene(pkg, tmp_path)
    assert scene.desc.n_meshes == 2
    check_deformations(pkg, scene, [0, 1], "ties")


def test_tree_small_meshes(pkg, tmp_path):
    for name, (v, f) in small_meshes().items():
        scene = obj_scene(pkg, tmp_path, name, v, f)
        got = assert_build_equals_host(pkg, scene, 0, scene, name)
        if name.startswith("coincident"):
            assert got["n_bvh_nodes"] == 2 and got["bvh_depth"] == 1, name + ": up to 8 inseparable triangles are one leaf"
    # nine coincident triangles are halved as they stand
    v, f = coincident(9)
    scene = obj_scene(pkg, tmp_path, "coincident9", v, f)
    assert assert_build_equals_host(pkg, scene, 0, scene, "coincident9")["n_bvh_nodes"] == 4


def test_tree_nan_vertices(pkg, golden, tmp_path):
    from test_gpu_scene_update import torus_scene
    for tag, scene in (("teapot", golden("teapot2_240x135").scene(pkg)), ("torus", torus_scene(pkg, tmp_path))):
        for name, v in nan_variants(scene.mesh_vertices(0)).items():
            now = clone(pkg, scene)
            now.set_mesh_vertices(0, v)
            got = assert_build_equals_host(pkg, scene, 0, now, "%s, %s" % (tag, name))
            if name == "v[0] NaN":
                assert np.isnan(got["bmin"]).all() and np.isnan(got["bmax"]).all()
            else:
                assert not np.isnan(got["bmin"]).any()


def test_tree_unreferenced_vertex(pkg, tmp_path):
    v, f = soup(7, 3)
    v = np.concatenate([v, np.array([[50, -60, 70]], np.float32)])  # in the mesh box, in no triangle
    scene = obj_scene(pkg, tmp_path, "loose", v, f)
    got = assert_build_equals_host(pkg, scene, 0, scene, "an unreferenced vertex")
    assert got["bmax"][0] == 50 and got["bmax"][2] == 70 and got["bmin"][1] == -60
    root = got["ref_bvh"][1].view(np.float32)
    assert root[4] < 3 and root[6] < 3, "the tree's root box took the unreferenced vertex"


def test_deep_row_is_deeper_than_the_walk_stack(pkg, tmp_path):
    """60 triangles with centres at 0.5^k: the host builds 57 levels (more than RTU_MAX_BVH_STACK, the case rtu_update_meshes_device can
    only refuse after the build) and the host form, which has no bound, the same tree."""
    v, f = deep_row()
    scene = obj_scene(pkg, tmp_path, "deep", v, f)
    assert scene.mesh(0).bvh_depth > RTU_MAX_BVH_STACK == 48
    got = assert_build_equals_host(pkg, scene, 0, scene, "deep row")
    assert got["bvh_depth"] == scene.mesh(0).bvh_depth == 57
    # the same connectivity laid out evenly is shallow: what the GPU test uploads before it deforms into the deep row
    fv, ff = flat_row()
    assert np.array_equal(ff, f)
    flat = obj_scene(pkg, tmp_path, "flat", fv, ff)
    assert flat.mesh(0).bvh_depth <= 8
    now = clone(pkg, flat)
    now.set_mesh_vertices(0, v)
    assert assert_build_equals_host(pkg, flat, 0, now, "flat row -> deep row")["bvh_depth"] == 57


# ---- 3. normals -------------------------------------------------------------------------------------------------------------------

def normals_mesh():
    """A torus patch without vn lines, one face naming a vertex twice, one vertex in no face."""
    nu, nv_ = 9, 5
    v = []
    for i in range(nu + 1):
        for j in range(nv_ + 1):
            a, b = 2 * np.pi * i / nu, 2 * np.pi * j / nv_
            v.append(((2 + 0.7 * np.cos(b)) * np.cos(a), (2 + 0.7 * np.cos(b)) * np.sin(a), 0.7 * np.sin(b)))
    f = []
    for i in range(nu):
        for j in range(nv_):
            p = i * (nv_ + 1) + j
            f += [(p, p + nv_ + 1, p + nv_ + 2), (p, p + nv_ + 2, p + 1)]
    f.append((3, 3, 10))  # names vertex 3 twice: its zero cross product is added twice
    v.append((9, 9, 9))   # no face: 0 / 0
    return np.array(v, np.float32), np.array(f)


def vn_of(scene, mesh):
    m = scene.mesh(mesh)
    return np.ctypeslib.as_array(ctypes.cast(m.vn, ctypes.POINTER(ctypes.c_float)), (m.nvn, 3)).copy()


def test_normals_by_adjacency_equal_compute_normals(pkg, tmp_path):
    v, f = normals_mesh()
    scene = obj_scene(pkg, tmp_path, "patch", v, f, normals=False)  # the loader ran ComputeNormals
    m = scene.mesh(0)
    assert m.nvn == m.nv
    want = vn_of(scene, 0)
    assert np.isnan(want[-1]).all() and not np.isnan(want[:-1]).any()
    got = pkg.host_ref_build(scene, 0)["vn"]
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "normals differ at %d floats" % int((got.view(np.uint32) != want.view(np.uint32)).sum())
    for d in DEFORMATIONS:
        now = deformed_scene(pkg, scene, 0, d)
        now.recompute_normals(0)
        got = pkg.host_ref_build(scene, 0, now.mesh_vertices(0))["vn"]
        assert np.array_equal(got.view(np.uint32), vn_of(now, 0).view(np.uint32)), deform_name(d)
    # a mesh with normals of its own has no such form
    own = obj_scene(pkg, tmp_path, "own", *soup(3, 1))
    own.mesh(0).nvn -= 1
    n = ctypes.c_size_t(0)
    assert pkg.hip.rtu_debug_host_ref_build(own.desc.meshes, None, 7, None, 0, ctypes.byref(n)) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_debug_host_ref_build(None, None, 4, None, 0, ctypes.byref(n)) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_debug_host_ref_build(scene.desc.meshes, None, 99, None, 0, ctypes.byref(n)) == pkg.RTU_ERR_ARG
