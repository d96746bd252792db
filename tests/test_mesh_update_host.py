"""Deforming a loaded mesh on the host (rtu_scene_set_mesh_vertices / rtu_scene_recompute_normals) and the host restatement of what
rtu_update_meshes writes on the device (rtu_debug_host_mesh). No GPU.

  * an edited scene is, byte for byte as a blob, the scene a load of an .obj with the deformed vertices gives;
  * the refit of the collapsed fast trees keeps every ref word and the element order of the uploaded mesh, and each child box is the
    exact min / max of the vertices it stands for; triangle records equal a numpy restatement of build_tri_records bit for bit.

The deformations are defined here once (test_gpu_mesh_update.py imports them)."""
import ctypes
import math
import os
import re
import shutil

import numpy as np
import pytest

from conftest import MAC_PREFIX, REPO

RTU_MAX_BVH_STACK = int(re.search(r"#define RTU_MAX_BVH_STACK\s+(\d+)", open(os.path.join(REPO, "include", "rtu_scene.h")).read()).group(1))

# name, argument. The last two make coplanar and zero-area triangles (exact ties, NaN normals) by the thousand: they test the
# builders here; images of flat and welded meshes are rendered from tests/scenes/ties (test_gpu_ties.py).
DEFORMATIONS = [("wobble", 0), ("wobble", 1), ("wobble", 2), ("twist", 30), ("twist", 60), ("twist", 120), ("bulge", None),
                ("flatten", None), ("collapse", None)]
RENDERED = [("wobble", 0), ("wobble", 1), ("wobble", 2), ("twist", 120), ("bulge", None)]
EMPTY_REF = 0x0FFFFFFF


def deform_name(d):
    return d[0] if d[1] is None else "%s%d" % d


def deform(v, lo, hi, name, arg=None):
    """The deformed positions of v [nv, 3]: computed in float64 from the mesh's own bounding box lo / hi, rounded to float32."""
    p = np.asarray(v, np.float64).copy()
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    c = 0.5 * (lo + hi)
    r = float(np.max(0.5 * (hi - lo)))
    t = (p[:, 2] - lo[2]) / (hi[2] - lo[2])
    if name == "wobble":
        p[:, 2] += 0.05 * r * np.sin(6.0 * (p[:, 0] - c[0]) / r + 0.9 * arg)
    elif name == "twist":
        a = math.radians(arg) * t
        x, y = p[:, 0] - c[0], p[:, 1] - c[1]
        p[:, 0] = c[0] + x * np.cos(a) - y * np.sin(a)
        p[:, 1] = c[1] + x * np.sin(a) + y * np.cos(a)
    elif name == "bulge":
        s = 1.0 + 0.6 * np.sin(math.pi * t)
        p[:, 0] = c[0] + (p[:, 0] - c[0]) * s
        p[:, 1] = c[1] + (p[:, 1] - c[1]) * s
    elif name == "flatten":
        p[:, 2] = lo[2]
    elif name == "collapse":
        p[:] = c
    else:
        raise ValueError(name)
    return p.astype(np.float32)


def clone(pkg, scene):
    return pkg.Scene(pkg.host.rtu_scene_clone(scene.desc_ptr))


def deformed_vertices(scene, mesh, d):
    m = scene.mesh(mesh)
    return deform(scene.mesh_vertices(mesh), list(m.bound_min), list(m.bound_max), *d)


def deformed_scene(pkg, scene, mesh, d):
    """A copy of `scene` with mesh `mesh` deformed in place (set_mesh_vertices)."""
    out = clone(pkg, scene)
    out.set_mesh_vertices(mesh, deformed_vertices(scene, mesh, d))
    return out


def rewrite_obj_vertices(src, dst, v, keep_normals=True):
    """The .obj `src` with its k-th `v` line replaced by v[k] (%.9g round-trips every float32); keep_normals False: without its vn
    lines and the normal fields of its faces."""
    k = 0
    with open(src) as f, open(dst, "w") as g:
        for line in f:
            w = line.split()
            if w and w[0] == "v":
                g.write("v %.9g %.9g %.9g\n" % tuple(float(x) for x in v[k]))
                k += 1
            elif w and w[0] == "vn" and not keep_normals:
                continue
            elif w and w[0] == "f" and not keep_normals:
                g.write("f " + " ".join(x.split("/")[0] for x in w[1:]) + "\n")
            else:
                g.write(line)
    assert k == len(v)


def mesh_arrays(scene, mesh):
    """f [nf, 3], v [nv, 3] of a mesh."""
    m = scene.mesh(mesh)
    f = np.ctypeslib.as_array(ctypes.cast(m.f, ctypes.POINTER(ctypes.c_uint32)), (m.nf, 3)).copy()
    return f, scene.mesh_vertices(mesh)


# ---- 1. set_mesh_vertices equals a load -------------------------------------------------------------------------------------------

def check_edit_equals_load(pkg, load, obj_path, pristine_obj, tmp, recompute=False):
    """load(): the scene from its files as they are now. For every deformation: the scene edited in place has the blob bytes of a load
    of the files with the deformed vertices written into the .obj."""
    shutil.copyfile(pristine_obj, obj_path)
    base = load()
    assert base.desc.n_meshes == 1
    nodes = set()
    for d in DEFORMATIONS:
        v = deformed_vertices(base, 0, d)
        rewrite_obj_vertices(pristine_obj, obj_path, v)
        want = load()
        # a property of these inputs (the device path needs it), not a skip
        assert want.mesh(0).bvh_depth <= RTU_MAX_BVH_STACK, "%s: depth %d" % (deform_name(d), want.mesh(0).bvh_depth)
        got = clone(pkg, base)
        got.set_mesh_vertices(0, v)
        if recompute:
            got.recompute_normals(0)
        assert got.to_blob_bytes() == want.to_blob_bytes(), "%s: the edited scene is not the loaded one" % deform_name(d)
        assert got.to_blob_bytes() != base.to_blob_bytes()
        nodes.add(want.mesh(0).n_bvh_nodes)
        print("%s: %d nodes, depth %d" % (deform_name(d), want.mesh(0).n_bvh_nodes, want.mesh(0).bvh_depth))
    return base, nodes


def test_set_mesh_vertices_equals_a_load_teapot(pkg, scene_files, tmp_path):
    root = tmp_path / "root"
    shutil.copytree(os.path.join(scene_files, "SceneFiles", "Project7"), str(root / "SceneFiles" / "Project7"))
    obj = str(root / "SceneFiles" / "Project7" / "teapot.obj")
    pristine = str(tmp_path / "pristine.obj")
    shutil.copyfile(obj, pristine)
    load = lambda: pkg.Scene.from_xml(str(root / "SceneFiles" / "Project7" / "scene.xml"), MAC_PREFIX, str(root))
    base, nodes = check_edit_equals_load(pkg, load, obj, pristine, tmp_path)
    assert len(nodes) > 1, "no deformation changed the size of the reference's tree"
    # the teapot's file carries its own normals: recompute_normals refuses and changes no byte
    before = base.to_blob_bytes()
    assert pkg.host.rtu_scene_recompute_normals(base._h, 0) == -1
    assert pkg.host.rtu_host_last_error().decode()
    assert base.to_blob_bytes() == before
    # new normals travel with the vertices
    v = deformed_vertices(base, 0, ("wobble", 1))
    m = base.mesh(0)
    vn = np.ctypeslib.as_array(ctypes.cast(m.vn, ctypes.POINTER(ctypes.c_float)), (m.nvn, 3)).copy()
    vn2 = np.roll(vn, 1, axis=1)
    a, b = clone(pkg, base), clone(pkg, base)
    a.set_mesh_vertices(0, v)
    b.set_mesh_vertices(0, v, vn2)
    ma = a.mesh(0)
    mb = b.mesh(0)
    got = np.ctypeslib.as_array(ctypes.cast(mb.vn, ctypes.POINTER(ctypes.c_float)), (mb.nvn, 3))
    kept = np.ctypeslib.as_array(ctypes.cast(ma.vn, ctypes.POINTER(ctypes.c_float)), (ma.nvn, 3))
    assert np.array_equal(got, vn2) and np.array_equal(kept, vn)


def test_set_mesh_vertices_equals_a_load_torus(pkg, tmp_path):
    from test_gpu_scene_update import torus_scene
    torus_scene(pkg, tmp_path)  # writes torus.obj and s.xml
    obj = str(tmp_path / "torus.obj")
    pristine = str(tmp_path / "pristine.obj")
    shutil.copyfile(obj, pristine)
    check_edit_equals_load(pkg, lambda: pkg.Scene.from_xml(str(tmp_path / "s.xml")), obj, pristine, tmp_path)


def test_recompute_normals_equals_a_load(pkg, tmp_path):
    from test_gpu_scene_update import torus_scene
    torus_scene(pkg, tmp_path)
    obj = str(tmp_path / "torus.obj")
    pristine = str(tmp_path / "pristine.obj")
    f, v = mesh_arrays(pkg.Scene.from_xml(str(tmp_path / "s.xml")), 0)
    rewrite_obj_vertices(obj, pristine, v, keep_normals=False)  # a file without vn lines: the loader computes the normals
    check_edit_equals_load(pkg, lambda: pkg.Scene.from_xml(str(tmp_path / "s.xml")), obj, pristine, tmp_path, recompute=True)


def test_bad_arguments(pkg, golden):
    scene = golden("teapot2_240x135").scene(pkg)
    before = scene.to_blob_bytes()
    v = scene.mesh_vertices(0)
    assert pkg.host.rtu_scene_set_mesh_vertices(scene._h, 1, v.ctypes.data, None) == -1
    assert "no mesh 1" in pkg.host.rtu_host_last_error().decode()
    assert pkg.host.rtu_scene_set_mesh_vertices(scene._h, 0, None, None) == -1
    assert pkg.host.rtu_scene_set_mesh_vertices(None, 0, v.ctypes.data, None) == -1
    assert pkg.host.rtu_scene_recompute_normals(scene._h, 7) == -1
    assert pkg.host.rtu_scene_recompute_normals(None, 0) == -1
    with pytest.raises(pkg.RtuError):
        scene.set_mesh_vertices(0, v[:-1])
    assert scene.to_blob_bytes() == before
    scene.set_mesh_vertices(0, v)  # the same vertices: the same scene
    assert scene.to_blob_bytes() == before


# ---- 2. the host refit ------------------------------------------------------------------------------------------------------------

def wide_slots(tree, width):
    """lo [n, W, 3], hi [n, W, 3], ref [n, W] of a collapsed tree as host_mesh() / Context.mesh_arrays() return it."""
    u = tree.view(np.uint32)
    if width == 4:
        return tree[:, 0:3, :].transpose(0, 2, 1), tree[:, 3:6, :].transpose(0, 2, 1), u[:, 6, :]
    return tree[:, 0::2, 0:3], tree[:, 1::2, 0:3], u[:, 0::2, 3]


def tri_records_numpy(f, v, elements):
    """build_tri_records (rtu_meshrec.h: mu_tri_record) restated in numpy float32, one rounding per operation: [n, 16] float32."""
    f32 = np.float32
    with np.errstate(all="ignore"):
        A, B, C = (v[f[elements, k]].astype(f32) for k in range(3))
        p, q = B - A, C - A
        cr = np.stack([p[:, 1] * q[:, 2] - p[:, 2] * q[:, 1], p[:, 2] * q[:, 0] - p[:, 0] * q[:, 2], p[:, 0] * q[:, 1] - p[:, 1] * q[:, 0]], axis=1)
        ln = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
        N = cr / ln[:, None]
        an = np.abs(N)
        smax = lambda a, b: np.where(a < b, b, a)
        mx = smax(smax(an[:, 0], an[:, 1]), an[:, 2])
        axis = np.where(mx == an[:, 0], 0, np.where(mx == an[:, 1], 1, 2)).astype(np.uint32)
        px = lambda P: np.where(axis == 0, P[:, 1], P[:, 0])
        py = lambda P: np.where(axis == 2, P[:, 1], P[:, 2])
        ax, ay, bx, by, cx, cy = px(A), py(A), px(B), py(B), px(C), py(C)
        e1x, e1y, e2x, e2y = cx - ax, cy - ay, bx - ax, by - ay
        area = (((-e1y) * e2x + e1x * e2y).astype(np.float64) / 2.0).astype(f32)
        rcp = (1.0 / area.astype(np.float64)).view(np.uint64)
    out = np.zeros((len(elements), 16), f32)
    out[:, 0:3] = A
    out[:, 3:6] = N
    out[:, 6], out[:, 7] = ax, ay
    out[:, 8], out[:, 9], out[:, 10], out[:, 11] = e1x, e1y, e2x, e2y
    o = out.view(np.uint32)
    o[:, 12] = (rcp & 0xFFFFFFFF).astype(np.uint32)
    o[:, 13] = (rcp >> 32).astype(np.uint32)
    o[:, 14] = axis
    return out


def same_bits_nan(a, b):
    """Bit for bit, NaN equal to NaN."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))


def assert_same_structures(got, want, what, strict_nan=False):
    """Two mesh dumps: integers and ref words exactly, boxes as float VALUES (-0 = +0: which of them a tie keeps depends on the order of
    a reduction and changes no ray), records bit for bit — NaN equal to NaN unless strict_nan."""
    for width, key in ((4, "bvh4"), (8, "bvh8")):
        glo, ghi, gref = wide_slots(got[key], width)
        wlo, whi, wref = wide_slots(want[key], width)
        assert got[key].shape == want[key].shape, "%s: %s has another size" % (what, key)
        assert np.array_equal(gref, wref), "%s: ref words of %s differ" % (what, key)
        assert np.array_equal(glo, wlo) and np.array_equal(ghi, whi), "%s: boxes of %s differ at %d floats" % (
            what, key, int((glo != wlo).sum() + (ghi != whi).sum()))
    for key in ("fast_elements", "ref_elements", "ref_bvh"):
        assert np.array_equal(got[key], want[key]), "%s: %s differs" % (what, key)
    for key in ("fast_tri", "ref_tri"):
        same = np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)) if strict_nan else same_bits_nan(got[key], want[key])
        assert same, "%s: %s differs" % (what, key)
    for key in ("v", "vn", "bmin", "bmax"):
        assert np.array_equal(got[key].view(np.uint32), want[key].view(np.uint32)), "%s: %s differs" % (what, key)
    assert np.float32(got["scale"]).view(np.uint32) == np.float32(want["scale"]).view(np.uint32), "%s: scale differs" % what
    assert got["n_bvh_nodes"] == want["n_bvh_nodes"] and got["any_empty_box"] == want["any_empty_box"], "%s: header differs" % what


def check_boxes_are_exact(dump, f, v, what):
    """Every leaf slot's box is the exact min / max of the vertices of its element slots, every inner slot's the union of the boxes of
    the node it refers to — so every triangle lies inside its leaf slot and every child node inside the slot that refers to it."""
    el = dump["fast_elements"]
    for width, key in ((4, "bvh4"), (8, "bvh8")):
        lo, hi, ref = wide_slots(dump[key], width)
        n = len(ref)
        for i in range(n - 1, -1, -1):
            for c in range(width):
                r = int(ref[i, c])
                if r == EMPTY_REF:
                    assert np.all(np.isinf(lo[i, c])) and np.all(np.isinf(hi[i, c]))
                elif r >> 28:
                    first, count = r & 0x0FFFFFFF, r >> 28
                    assert count <= width and first + count <= len(el)
                    pts = v[f[el[first:first + count]].reshape(-1)]
                    assert np.array_equal(lo[i, c], pts.min(axis=0)) and np.array_equal(hi[i, c], pts.max(axis=0)), \
                        "%s: %s node %d slot %d is not the box of its triangles" % (what, key, i, c)
                else:
                    assert i < r < n, "%s: %s node %d slot %d refers to node %d" % (what, key, i, c, r)
                    used = ref[r] != EMPTY_REF
                    assert np.array_equal(lo[i, c], lo[r][used].min(axis=0)) and np.array_equal(hi[i, c], hi[r][used].max(axis=0)), \
                        "%s: %s node %d slot %d is not the union of node %d" % (what, key, i, c, r)


@pytest.mark.parametrize("tag", ["teapot2_240x135", "p13_200x150", "p5low_200x150"])
def test_host_refit(pkg, golden, tag):
    scene = golden(tag).scene(pkg)
    assert scene.desc.n_meshes >= 1
    for mesh in range(scene.desc.n_meshes):
        f, v = mesh_arrays(scene, mesh)
        plain = pkg.host_mesh(scene, mesh)
        what = "%s mesh %d" % (tag, mesh)
        # a refit with the uploaded vertices reproduces the build
        assert_same_structures(pkg.host_mesh(scene, mesh, scene), plain, what + " refit in place")
        check_boxes_are_exact(plain, f, v, what)
        assert same_bits_nan(plain["fast_tri"].reshape(-1, 16), tri_records_numpy(f, v, plain["fast_elements"]))
        assert same_bits_nan(plain["ref_tri"].reshape(-1, 16), tri_records_numpy(f, v, plain["ref_elements"]))
        for d in DEFORMATIONS:
            check_refit(pkg, scene, mesh, deformed_scene(pkg, scene, mesh, d), plain, "%s %s" % (what, deform_name(d)))


def check_refit(pkg, scene, mesh, now, plain, w):
    """`plain`: host_mesh(scene, mesh). The refit of that upload to the vertices of `now` keeps the uploaded topology; boxes, records,
    vertices and `ref` tree are those of `now`."""
    f, _ = mesh_arrays(scene, mesh)
    got = pkg.host_mesh(scene, mesh, now)
    f2, v2 = mesh_arrays(now, mesh)
    assert np.array_equal(f2, f)
    # the topology is the uploaded mesh's
    for width, key in ((4, "bvh4"), (8, "bvh8")):
        assert np.array_equal(wide_slots(got[key], width)[2], wide_slots(plain[key], width)[2]), "%s: ref words of %s moved" % (w, key)
    assert np.array_equal(got["fast_elements"], plain["fast_elements"]), "%s: fast.elements moved" % w
    # boxes, records, vertices and `ref` tree are the deformed mesh's
    check_boxes_are_exact(got, f, v2, w)
    assert same_bits_nan(got["fast_tri"].reshape(-1, 16), tri_records_numpy(f, v2, plain["fast_elements"])), "%s: fast.tri" % w
    rebuilt = pkg.host_mesh(now, mesh)
    for key in ("ref_bvh", "ref_elements", "v", "vn", "bmin", "bmax"):
        assert np.array_equal(got[key].view(np.uint32), rebuilt[key].view(np.uint32)), "%s: %s is not the deformed mesh's" % (w, key)
    assert same_bits_nan(got["ref_tri"].reshape(-1, 16), tri_records_numpy(f, v2, rebuilt["ref_elements"])), "%s: ref.tri" % w
    assert got["n_bvh_nodes"] == now.mesh(mesh).n_bvh_nodes and got["any_empty_box"] == rebuilt["any_empty_box"]


def test_host_refit_of_a_flat_upload(pkg, tmp_path):
    """The inverse direction: the scene uploaded FLAT (tests/scenes/ties: a torus with every z = 0, so build_wide4 / build_wide8 choose
    their collapses by box area with every area zero) and refitted to the round torus, which inflates that topology — and to the
    half-welded pancake (zero-area triangles, NaN records). Leaf and inner boxes are still the exact min / max, every ref word is kept."""
    from test_ties_host import pancake, round_vertices, ties_scene, welded_vertices, with_vertices
    flat = ties_scene(pkg, tmp_path)
    mesh = pancake(flat)
    f, v = mesh_arrays(flat, mesh)
    assert np.all(v[:, 2] == 0) and list(flat.mesh(mesh).bound_min)[2] == 0 == list(flat.mesh(mesh).bound_max)[2]
    plain = pkg.host_mesh(flat, mesh)
    assert_same_structures(pkg.host_mesh(flat, mesh, flat), plain, "pancake refit in place")
    check_boxes_are_exact(plain, f, v, "pancake")
    for width, key in ((4, "bvh4"), (8, "bvh8")):  # every box of the flat upload has no thickness
        lo, hi, ref = wide_slots(plain[key], width)
        used = ref != EMPTY_REF
        assert used.any() and np.all(lo[used][:, 2] == 0) and np.all(hi[used][:, 2] == 0)
    assert same_bits_nan(plain["fast_tri"].reshape(-1, 16), tri_records_numpy(f, v, plain["fast_elements"]))
    round_ = with_vertices(pkg, flat, mesh, round_vertices(v))
    welded = with_vertices(pkg, flat, mesh, welded_vertices(v))
    for now, name in ((round_, "round"), (welded, "welded")):
        assert now.mesh(mesh).bvh_depth <= RTU_MAX_BVH_STACK, "%s: depth %d" % (name, now.mesh(mesh).bvh_depth)  # a property of these inputs
        check_refit(pkg, flat, mesh, now, plain, "pancake -> " + name)
    assert np.isnan(pkg.host_mesh(flat, mesh, welded)["fast_tri"]).any(), "the welded pancake has no degenerate triangle"
    # ... and the direction the other tests take, on the same mesh: uploaded round, pressed flat
    check_refit(pkg, round_, mesh, flat, pkg.host_mesh(round_, mesh), "round -> pancake")


def test_host_mesh_refuses_another_shape(pkg, golden):
    a = golden("teapot2_240x135").scene(pkg)
    b = golden("p5low_200x150").scene(pkg)
    n = ctypes.c_size_t(0)
    size = ctypes.sizeof(pkg.RtuMesh)
    assert pkg.hip.rtu_debug_host_mesh(a.desc.meshes, b.desc.meshes, 0, None, 0, ctypes.byref(n)) == pkg.RTU_ERR_SCENE_SHAPE
    assert pkg.hip.rtu_debug_host_mesh(a.desc.meshes, None, 99, None, 0, ctypes.byref(n)) == pkg.RTU_ERR_ARG
    assert pkg.hip.rtu_debug_host_mesh(None, None, 0, None, 0, ctypes.byref(n)) == pkg.RTU_ERR_ARG
    assert size > 0
