"""Mirrored, stretched, cancelling and singular node transformations, on the oracle alone: the scene families of
tests/test_gpu_transforms.py, what each must contain to test anything, and the four of them that the compiled reference pins
(tests/scenes/transforms/t*.xml -> tests/golden/xf_t*_96x64, tests/golden/make_goldens.py).

Every conservative structure of the fast variant is derived from the node transformations (world_bounds, world_far and near_margin of
rtu_capi_build.hip; the rectangles and masks of k_prelude; the occluder lists of both builders). Every family is a compact scene —
a checkered floor 28 units wide, a point and a direct light, materials that are shiny, mirror, glass with absorption, checkered and
file-textured — with a sphere, a plane and the torus of tests/test_oracle_far.py (vertex normals, `vt` lines) under the class:

  T1  mirrored: one negative axis on a leaf of each kind (a glass sphere, a mirror card, a textured torus), two negative axes, a uniform
      negative scale (a torus, a card seen from behind), a group scaled x = -1 above rotated, non-uniformly scaled children
  T2  stretched: a needle (1e2) and a disc (1e3) sphere, a strip plane (1e2), a flattened (1e3) and a drawn-out (1e2) torus, each
      rotated after its scale; a sphere scaled (2.4, 2.4, 0.024) AFTER its rotation (a shear); a group scaled (20, 0.05, 1) and rotated
      above a torus and a sphere scaled (0.05, 20, 1): their world size is ordinary
  T3  cancelling chains: a group scaled by S, its children by 1 / S and rotated, S = 1e4, 1e-4 and, on the x axis alone, 1e25 and
      1e-25 (rotated about x); with S = 1e4 also a chain of seven nodes below the root (the deepest RTU_MAX_NODE_DEPTH allows) scaled 1e4, 1e-4,
      1e4, 1e-4, 1e4, 1, 8e-5
  T4  singular and overflowing: a scale of 0 on one axis of a sphere, of a mesh and of a group with three children; a sphere scaled
      by 1e-30 (its inverse overflows) and a plane scaled by 1e30 (the determinant overflows in the loader: itm is NaN too, but its
      corners are finite, so it alone has a node-level bound and takes the scene's scale to 1e30; "T4 compact" is T4 without it);
      ordinary objects beside them. No ray hits any of these nodes and the image is the image without them
  T5  at the switch: a group scaled (a, 1 / a, 1) and rotated above a card and a torus that undo it. K — and with it the far term at
      the scene's extent, D(2 wscale) — grows with a^2; a = 2.151 and 2.495 put D(2 wscale) at 0.9 and 1.1 times 12 * 1e-4 * wscale,
      where near_margin switches the far term on. (A stretch BEFORE a node's own rotation does not enter K: |R S| |S^-1 R^T| = |R| |R^T|.)
      `model_far` restates world_far and near_margin in numpy; test_the_occluder_lists_show_the_switch holds it against the builder

`transformed(scene, n_plain)` names the nodes under the class: every object node after the first n_plain (the floor and the ordinary
objects, which a family lists first). What the tests below print (96 x 64; node: first hits of camera rays):

  T1   nodes 2-7, 9-11: 82 147 229 71 108 80 209 66 91; from behind: node 7, 80 camera rays; secondary rays 1068 (0 without the nodes
       under the class), shadow rays 9312 (8856), 1457 pixels differ
  T2   nodes 3-8, 10, 11: 85 146 97 305 58 260 179 79; from behind: node 10, 51 rays of R2; secondary 1522 (0), shadow 9310 (8856), 1724 pixels
  T3   S = 1e4: nodes 3-6, 13: 140 188 167 94 85; from behind: node 5, 56 rays of R2; secondary 1103 (0), shadow 9536 (8856), 834 pixels
       S = 1e-4: 140 188 167 94; secondary 1097, shadow 9518, 722 pixels.  x1e-25: 140 188 239 85; secondary 1171, shadow 9492, 815 pixels
       x1e25: 140 188 239 85; 489 NaN pixels (the normals overflow); secondary 592, shadow 8942, 815 pixels
  T4   7 singular nodes (6 compact), 0 hits from the camera and from R1-R4; secondary 1026, shadow 9432 with and without them, 0 pixels differ
  T5   nodes 6, 7: 159 95; from behind: node 6, 34 rays of R2
  the reference's line, largest over the oracle's hits of camera rays and R2 on the nodes under the class, in units of the far term D(pm)
  and of the plain margin 1e-4 max(wscale, pm); K; D(2 wscale) in units of the switch; (hits, hits model_skips would skip) camera, R2:
       T1        0.0204  0.049   K 48.3    0.458 off  (1083, 0) (1613, 0)
       T2        0.00236 0.592   K 4638    46.9  on   (1209, 0) (2034, 0)
       T3 1e4    0.0162  0.13    K 162     1.53  on   (674, 0)  (1206, 0)
       T3 1e-4   0.021   0.0484  K 50.7    0.449 off  (589, 0)  (994, 0)
       T3 x1e-25 6.5e-27 0.0564  K 1.9e26  1.7e24 on  (652, 0)  (913, 0)
       T3 x1e25  7.1e-27 0.0575  K 1.8e26  1.6e24 on  (652, 0)  (420, 0)
       T5 below  0.00983 0.0456  K 99.2    0.9   off  (254, 0)  (293, 0)
       T5 above  0.00909 0.0516  K 121.2   1.1   on   (254, 0)  (293, 0)
  occluder-list entries (point, direct light) of the first mesh at 0.7 / 0.9 / 1.1 of the switch: 32589 32877 / 32589 32877 / 54487 52999
  (wlist = 14.2 wscale at 1.1). tests/test_light_lists.py: per usable list 960 floor points in the mesh's shadow (958-960 occluded in the
  oracle) and 3181-3186 rays checked, 978-1046 of which hit the mesh; the point light's list is dropped for x1e25 and x1e-25
"""
import math
import os

import numpy as np
import pytest

from conftest import REPO, instantiate_scene
from test_fuzz_host import family_r2, ray_families
from test_gpu_ray_query import nodes
from test_oracle_far import RTU_OBJ_PLANE, RTU_OBJ_SPHERE, RTU_OBJ_TRIMESH, model_skips, model_world_bounds, torus
from test_oracle_rays import BIG, frame_of, make_rays, valid  # noqa: F401  (BIG, make_rays: for the tests that import this module)

W, H = 96, 64
TAGS = {"T1": "xf_t1_96x64", "T2": "xf_t2_96x64", "T3": "xf_t3_96x64", "T4": "xf_t4_96x64"}  # family -> golden tag
FILES = {"T1": "t1.xml", "T2": "t2.xml", "T3": "t3.xml", "T4": "t4.xml"}                      # ... -> tests/scenes/transforms/<file>
T3_S = ("1e4", "1e-4", "x1e25", "x1e-25")

MATERIALS = (
    '<material type="blinn" name="floor"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.15" g="0.2" b="0.5"/><color2 r="0.9" g="0.85" b="0.7"/>'
    '<scale value="0.125"/></diffuse><specular value="0.1"/><glossiness value="20"/></material>\n'
    '<material type="blinn" name="shiny"><diffuse r="0.8" g="0.25" b="0.2"/><specular value="0.7"/><glossiness value="40"/></material>\n'
    '<material type="blinn" name="mirror"><diffuse r="0.1" g="0.1" b="0.1"/><specular value="0.8"/><glossiness value="60"/><reflection value="0.8"/></material>\n'
    '<material type="blinn" name="glass"><diffuse r="0.05" g="0.05" b="0.05"/><specular value="0.9"/><glossiness value="100"/>'
    '<refraction index="1.5" value="0.9"/><absorption r="0.05" g="0.02" b="0.08"/></material>\n'
    '<material type="blinn" name="checker"><diffuse r="1" g="1" b="1" texture="checkerboard"><color1 r="0.1" g="0.6" b="0.3"/><color2 r="0.9" g="0.9" b="0.2"/>'
    '<scale value="0.2"/></diffuse><specular value="0.3"/><glossiness value="30"/></material>\n'
    '<material type="blinn" name="tiles"><diffuse r="1" g="1" b="1" texture="@DIR@/tiles.png"><scale x="0.5" y="0.5"/></diffuse><specular value="0.4"/>'
    '<glossiness value="50"/><reflection value="0.2"/></material>\n')
LIGHTS = ('<light type="ambient" name="amb"><intensity value="0.2"/></light>\n'
          '<light type="point" name="key"><intensity value="0.7"/><position x="-7" y="-11" z="15"/></light>\n'
          '<light type="direct" name="fill"><intensity value="0.4"/><direction x="0.4" y="0.5" z="-1"/></light>\n')
FLOOR = '<object type="plane" name="floor" material="floor"><scale value="14"/><translate z="-4"/></object>\n'
CAMERA = ('<camera><position x="1.5" y="-19" z="9"/><target x="0" y="-0.5" z="-2.5"/><up x="0" y="0" z="1"/><fov value="40"/>'
          '<width value="%d"/><height value="%d"/></camera>' % (W, H))
MESH = '@DIR@/torus.obj'


def obj(kind, name, material, xf):
    if kind == "group":
        return '<object name="%s">%s</object>\n' % (name, xf)
    if kind == "obj":
        return '<object type="obj" name="%s" material="%s">%s</object>\n' % (MESH, material, xf)
    return '<object type="%s" name="%s" material="%s">%s</object>\n' % (kind, name, material, xf)


def sc(x, y=None, z=None):
    return '<scale value="%s"/>' % x if y is None else '<scale x="%s" y="%s" z="%s"/>' % (x, y, z)


def rot(angle, x=0, y=0, z=0):
    return '<rotate angle="%s" x="%s" y="%s" z="%s"/>' % (angle, x, y, z)


def tr(x, y, z):
    return '<translate x="%s" y="%s" z="%s"/>' % (x, y, z)


def document(plain, special):
    return "<xml>\n<scene>\n%s%s%s%s%s</scene>\n%s\n</xml>\n" % (FLOOR, "".join(plain), "".join(special), MATERIALS, LIGHTS, CAMERA)


# ---- the families: name -> (XML of the ordinary objects after the floor, XML of the objects under the class) ---------------------------
def t1(benign=False):
    """benign: every scale positive (|s|), the scene the update test starts from."""
    m = (lambda s: s.replace("-", "")) if benign else (lambda s: s)
    special = [
        obj("sphere", "glass ball", "glass", m(sc("-1.5", "1", "0.8")) + rot(30, z=1) + tr(-6.5, -3, -2.9)),
        obj("plane", "mirror card", "mirror", m(sc("2.2", "-1.6", "1")) + rot(75, x=1) + rot(-20, z=1) + tr(-2, 4, -2.2)),
        obj("obj", "", "tiles", m(sc("0.9", "0.9", "-1.2")) + rot(35, x=1, y=0.3) + tr(2.5, -2, -2.6)),
        obj("sphere", "two axes", "checker", m(sc("-1.3", "-1.6", "1")) + rot(20, y=1) + tr(7.5, 1.5, -2.9)),
        obj("obj", "", "shiny", m(sc("-0.75")) + rot(60, x=1) + tr(-7, 4.5, -1.5)),
        obj("plane", "uniform card", "checker", m(sc("-1.5")) + rot(80, x=1) + rot(25, z=1) + tr(6, 6, -2.4)),
        obj("group", "mirrored group", "", m(sc("-1", "1", "1")) + rot(15, z=1) + tr(0.5, -6.5, -2.2) +
            obj("obj", "", "checker", sc("0.6", "0.9", "0.5") + rot(40, x=0.3, y=1, z=0.2) + tr(-4.5, 0, -0.6)) +
            obj("sphere", "in group", "mirror", sc("1.1", "0.6", "0.8") + rot(50, z=1) + tr(0.5, -1, -0.9)) +
            obj("plane", "in group", "tiles", sc("1.3", "0.8", "1") + rot(65, x=1) + rot(30, z=1) + tr(3.5, 1.5, -0.8))),
    ]
    return [], special


def t2(benign=False):
    """benign: aspect 1 everywhere. The thin ones lie near the camera and face it: a pixel is a quarter of a unit there."""
    def s(x, y, z):
        return sc(1, 1, 1) if benign else sc(x, y, z)
    special = [
        obj("sphere", "needle", "shiny", s(8, 0.08, 0.08) + rot(12, y=1, z=0.5) + tr(-1, -10, -0.5)),
        obj("sphere", "disc", "glass", s(2.5, 2.5, 0.0025) + rot(50, x=1, y=0.3) + tr(-7, 0.5, -1.8)),
        obj("plane", "strip", "checker", s(8, 0.08, 1) + rot(60, x=1) + rot(8, y=1) + tr(0, -8, 0.8)),
        obj("obj", "", "tiles", s(1.1, 1.1, 0.0011) + rot(40, x=1, z=0.2) + tr(6.5, 1, -2)),
        obj("obj", "", "mirror", s(3, 0.03, 0.03) + rot(55, x=1) + rot(-10, y=1) + tr(1, -9, -2)),
        obj("sphere", "sheared ball", "checker", ("" if benign else rot(40, x=1, y=1)) + s(2.4, 2.4, 0.024) + tr(-6.5, -5.5, -3.3)),
        obj("group", "stretched group", "", s(20, 0.05, 1) + rot(30, x=0.2, y=0.1, z=1) + tr(-1, 2.5, -2.4) +
            obj("obj", "", "checker", s(0.05, 20, 1)) +
            obj("sphere", "undone ball", "mirror", s(0.07, 28, 1.4) + (tr(4.5, 0, 1.5) if benign else tr(0.225, 0, 1.5)))),
    ]
    return [obj("sphere", "ball", "shiny", sc(1.0) + tr(7.5, -5, -3))], special


def t5(aspect):
    """A group scaled (a, 1 / a, 1) and rotated above a card and a torus that undo it: K grows with a^2 (the condition of the group's
    matrix times the children's 3 + 6 kappa), and nothing else in the scene changes."""
    a = float(aspect)
    plain = [obj("sphere", "ball", "glass", sc(1.2) + tr(-5, -3, -2.8)), obj("obj", "", "tiles", sc(0.8) + rot(30, x=1) + tr(4, -3, -2.6)),
             obj("sphere", "ball 2", "mirror", sc(1.1) + tr(6, 4, -2.9))]
    special = [obj("group", "stretched group", "", sc(repr(a), repr(1.0 / a), 1) + rot(35, x=1, y=0.2, z=1) + tr(-1, 3, -1.5) +
                   obj("plane", "undone card", "checker", sc(repr(2.0 / a), repr(2.0 * a), 1)) +
                   obj("obj", "", "shiny", sc(repr(0.7 / a), repr(0.7 * a), 0.7) + tr(repr(4.5 / a), 0, 1)))]
    return plain, special


def t3(S="1e4"):
    """A group scaled by S (on x alone for "x..."), children scaled by 1 / S and rotated (about x where S acts on x alone). A child's
    translation is given in the group's space: the world offset divided by S."""
    one_axis = S.startswith("x")
    s = S.lstrip("x")
    inv = ("1e-" + s[2:]) if "-" not in s else ("1e" + s[3:])
    f = float(inv)
    gs, cs = (sc(s, 1, 1), (lambda k: sc(repr(k * f), k, k))) if one_axis else (sc(s), (lambda k: sc(repr(k * f))))
    axis = dict(x=1) if one_axis else dict(x=0.3, y=1, z=0.4)

    def at(x, y, z):
        return tr(repr(x * f), y, z) if one_axis else tr(repr(x * f), repr(y * f), repr(z * f))
    special = [obj("group", "scaled group", "", gs + rot(20, z=1) + tr(-1, 0, -2) +
                   obj("sphere", "ball", "glass", cs(1.4) + rot(30, **axis) + at(-5, -3, -0.6)) +
                   obj("plane", "card", "mirror", cs(2.0) + rot(70, x=1) + at(0, 4.5, 0)) +
                   obj("obj", "", "tiles", cs(0.9) + rot(40, **axis) + at(3.5, -3, -0.5)) +
                   obj("sphere", "ball 2", "checker", cs(1.6) + rot(10, **axis) + at(7, 3, -0.4)))]
    if S == "1e4":
        chain = obj("obj", "", "shiny", sc("8e-5") + rot(55, x=1, y=0.2))
        for level in range(5, -1, -1):  # six groups above the leaf, seven nodes: 1e4, 1e-4, 1e4, 1e-4, 1e4, a rotation alone, 8e-5
            xf = ("" if level == 5 else sc("1e4") if level % 2 == 0 else sc("1e-4")) + rot(7 * (level + 1), z=1)
            chain = obj("group", "level %d" % level, "", xf + (tr(-7.5, 5, -1.6) if level == 0 else "") + chain)
        special.append(chain)
    return [], special


def t4(huge=True):
    plain = [obj("sphere", "ball", "glass", sc(1.3) + tr(-5, -3, -2.7)), obj("obj", "", "tiles", sc(0.9) + rot(35, x=1) + tr(2, -2, -2.5)),
             obj("plane", "card", "mirror", sc(2) + rot(75, x=1) + rot(-20, z=1) + tr(-2, 4, -2)), obj("sphere", "ball 2", "checker", sc(1.2) + tr(6.5, 3, -2.8))]
    special = [
        obj("sphere", "flat ball", "shiny", sc(1.5, 0, 1.5) + rot(20, z=1) + tr(-7, 2, -2)),
        obj("obj", "", "shiny", sc(1, 1, 0) + rot(30, x=1) + tr(5.5, -5, -2)),
        obj("group", "flat group", "", sc(0, 1, 1) + rot(10, z=1) + tr(0, -6, -2) +
            obj("sphere", "in flat", "shiny", sc(1.2)) + obj("obj", "", "checker", sc(0.6) + tr(3, 0, 0)) + obj("plane", "in flat", "mirror", rot(80, x=1) + tr(-3, 0, 0))),
        obj("sphere", "speck", "mirror", sc("1e-30") + tr(1, 1, -1)),
    ]
    if huge:  # its corners are finite, so it has a node-level bound: the scene's scale is then 1e30 and no margin culls anything
        special.append(obj("plane", "huge", "checker", sc("1e30") + rot(90, x=1) + tr(0, -40, 0)))
    return plain, special


FAMILIES = {"T1": t1, "T2": t2, "T3": t3, "T4": t4}


def family_xml(name, removed=False, **kw):
    """The scene text of a family with @DIR@ placeholders; removed: without the objects under the class."""
    if name.startswith("T5"):
        plain, special = t5(kw["aspect"])
    else:
        plain, special = FAMILIES[name](**kw)
    return document(plain, [] if removed else special), len(plain) + 1


def write_torus(path):
    """The torus of tests/test_oracle_far.py (24 x 10, vertex normals by finite differences as _write_uv_mesh takes them) with `vt`
    lines (u, v) and v/vt/vn faces: the reference reads the texture coordinates of every accepted hit."""
    nu, nv = 24, 10
    out, faces = [], []
    pts = [(i / nu, j / nv) for i in range(nu + 1) for j in range(nv + 1)]
    for u, v in pts:
        out.append("v %r %r %r\n" % tuple(torus(u, v)))
    for u, v in pts:
        out.append("vt %r %r\n" % (u, v))
    for u, v in pts:
        du = [a - b for a, b in zip(torus(u + 1e-4, v), torus(u - 1e-4, v))]
        dv = [a - b for a, b in zip(torus(u, v + 1e-4), torus(u, v - 1e-4))]
        n = (du[1] * dv[2] - du[2] * dv[1], du[2] * dv[0] - du[0] * dv[2], du[0] * dv[1] - du[1] * dv[0])
        ln = math.sqrt(sum(c * c for c in n)) or 1.0
        out.append("vn %r %r %r\n" % tuple(c / ln for c in n))
    for i in range(nu):
        for j in range(nv):
            a = i * (nv + 1) + j + 1
            b, c, d = a + 1, a + nv + 1, a + nv + 2
            faces += [(a, c, b), (b, c, d)]
    out += ["f %d/%d/%d %d/%d/%d %d/%d/%d\n" % (i, i, i, j, j, j, k, k, k) for i, j, k in faces]
    with open(str(path), "w") as f:
        f.write("".join(out))


def assets_dir(tmp):
    """tests/scenes/transforms copied to tmp with its placeholders filled in (torus.obj, the four pinned scenes), and the file texture
    they name, which is multimtl's."""
    import shutil
    instantiate_scene("transforms/t1.xml", tmp)
    shutil.copyfile(os.path.join(REPO, "tests", "scenes", "multimtl", "tiles.png"), os.path.join(str(tmp), "tiles.png"))
    return tmp


def load(pkg, d, name, removed=False, file=None, **kw):
    """-> (scene, number of object nodes that are not under the class). d: a directory made by assets_dir."""
    text, n_plain = family_xml(name, removed, **kw)
    path = os.path.join(str(d), file or "%s%s%s.xml" % (name, "_removed" if removed else "", "".join("_%s" % v for v in kw.values())))
    with open(path, "w") as f:
        f.write(text.replace("@DIR@", str(d)))
    return pkg.Scene.from_xml(path), n_plain


# the scenes of the GPU tests: label -> (family, keyword arguments)
SCENES = {"T1": ("T1", {}), "T2": ("T2", {}), "T4": ("T4", {}), "T4 compact": ("T4", {"huge": False})}
SCENES.update({"T3 S=%s" % S: ("T3", {"S": S}) for S in T3_S})


# ---- which nodes are under the class ------------------------------------------------------------------------------------------------
def object_nodes(scene):
    return [i for i in range(scene.desc.n_nodes) if nodes(scene)[i].obj_type in (RTU_OBJ_SPHERE, RTU_OBJ_PLANE, RTU_OBJ_TRIMESH)]


def transformed(scene, n_plain):
    return object_nodes(scene)[n_plain:]


def singular(scene, k):
    """Does the chain of node k hold an inverse that is not finite, or one that is zero (a scale of 1e30 has the inverse 1e-30, whose
    products with a direction underflow)?"""
    nd = nodes(scene)
    while k >= 0:
        itm = np.array(list(nd[k].itm), np.float64)
        if not np.isfinite(itm).all():
            return True
        k = nd[k].parent
    return False


# ---- world_far and near_margin (rtu_capi_build.hip), restated -----------------------------------------------------------------------
def abs_row_norm(m):
    return float(np.abs(m).sum(axis=1).max())


def model_far(scene):
    """K, Omega, wnoise, D(2 wscale) and what near_margin makes of them: dict(K, omega, wscale, wnoise, DP, on, near_m0, near_c1, wlist)."""
    nd = nodes(scene)
    u, K, omega = 2.0 ** -24, 0.0, 0.0
    for i in object_nodes(scene):
        ch, j = [], i
        while j >= 0:
            ch.append(j)
            j = nd[j].parent
        T, Ti, o, k_node, om = np.eye(3), np.eye(3), np.zeros(3), 0.0, 0.0
        for j in reversed(ch):  # root first
            tm = np.array(list(nd[j].tm), np.float64).reshape(3, 3).T
            itm = np.array(list(nd[j].itm), np.float64).reshape(3, 3).T
            k_node += abs_row_norm(T) * abs_row_norm(Ti) * (3.0 + 6.0 * abs_row_norm(np.abs(tm) @ np.abs(itm)))
            o = o + T @ np.array(list(nd[j].pos), np.float64)
            om = max(om, float(np.abs(o).max()))
            T, Ti = T @ tm, itm @ Ti
        if not (np.isfinite(k_node) and np.isfinite(om) and np.isfinite(abs_row_norm(T) * abs_row_norm(Ti))):
            continue
        K, omega = max(K, k_node), max(omega, om)
    _, scale = model_world_bounds(scene)
    ws = float(np.float32(scale))
    wn = float(np.float32(1.74 * u * K * (1 + 1e-6)))
    P, omega1 = 2.0 * ws, omega + 1.0
    f = lambda m: 1e-4 * max(ws, m) + wn * (m + omega1) * (m + ws)
    DP = wn * (P + omega1) * (P + ws)
    out = dict(K=K, omega=omega, wscale=ws, wnoise=wn, DP=DP, on=bool(DP >= 12.0 * 1e-4 * ws), near_m0=ws, near_c1=1e-4, wlist=ws)
    if out["on"]:
        c1 = f(P) / P * (1 + 1e-6)
        lo, hi = 0.0, P
        for _ in range(64):
            mid = 0.5 * (lo + hi)
            if c1 * mid >= f(mid):
                hi = mid
            else:
                lo = mid
        out.update(near_m0=min(hi * (1 + 1e-6), 1e30), near_c1=min(c1, 1e30), wlist=min((ws + 1e4 * DP) * (1 + 1e-6), 1e30))
    return out


def line_deviation(scene, k, rays, t):
    """How far, on its worst axis, the line that node k's object is tested against (Node::ToNodeCoords in binary32 down the chain,
    taken back to the world in binary64) is from the caller's line at parameter t."""
    from test_gpu_surface import to_node_chain
    from test_oracle_far import chain
    with np.errstate(all="ignore"):
        p, d = to_node_chain(scene, k, rays["org"], rays["dir"])
    q = p.astype(np.float64) + t[:, None] * d.astype(np.float64)
    for tm, pos in chain(scene, k):
        q = q @ tm.T + pos
    return np.abs(q - (rays["org"].astype(np.float64) + t[:, None] * rays["dir"].astype(np.float64))).max(axis=1)


def t5_aspect(pkg, d, ratio):
    """The aspect of T5's card at which D(2 wscale) = ratio * 12e-4 wscale (bisection on the restated constants)."""
    lo, hi = 1.0, 30.0
    for k in range(30):
        mid = math.sqrt(lo * hi)
        m = model_far(load(pkg, d, "T5", aspect=mid, file="t5_probe.xml")[0])
        if m["DP"] >= ratio * 12e-4 * m["wscale"]:
            hi = mid
        else:
            lo = mid
    return float(np.float32(hi))


T5_RATIOS = {"T5 below": 0.9, "T5 above": 1.1}


def t5_scene(pkg, d, which):
    return load(pkg, d, "T5", aspect=t5_aspect(pkg, d, T5_RATIOS[which]), file=which.replace(" ", "_") + ".xml")


def scene_of(pkg, d, label):
    if label.startswith("T5"):
        return t5_scene(pkg, d, label)
    name, kw = SCENES[label]
    return load(pkg, d, name, **kw)


def unit_rows(a):
    return a / np.linalg.norm(a, axis=1)[:, None]


# ==== fixtures ======================================================================================================================
@pytest.fixture(scope="module")
def xf_dir(tmp_path_factory):
    return assets_dir(tmp_path_factory.mktemp("transforms"))


def camera_hits(pkg, orc, scene):
    rays = pkg.camera_rays(frame_of(pkg, scene, W, H))
    assert valid(rays).all()
    return rays, orc.trace_rays(scene, rays, threads=8)


ALL = sorted(SCENES) + sorted(T5_RATIOS)


# ==== the committed scene files are the generator's ===================================================================================
@pytest.mark.parametrize("name", sorted(FILES))
def test_the_scene_files_are_what_the_generator_writes(name):
    assert open(os.path.join(REPO, "tests", "scenes", "transforms", FILES[name])).read() == family_xml(name)[0]


def test_the_torus_file_is_what_write_torus_writes(tmp_path):
    write_torus(tmp_path / "torus.obj")
    assert (tmp_path / "torus.obj").read_text() == open(os.path.join(REPO, "tests", "scenes", "transforms", "torus.obj")).read()


# ==== the oracle against the compiled reference ====================================================================================
@pytest.mark.parametrize("name", sorted(TAGS))
def test_oracle_bit_exact_vs_reference_golden(pkg, orc, golden, name):
    """As tests/test_oracle.py: z and linear RGB bit for bit, the counters equal, the 8-bit images the reference wrote."""
    g = golden(TAGS[name])
    assert (g.width, g.height) == (W, H)
    out, st = orc.render(g.scene(pkg), W, H, threads=4)
    assert np.array_equal(out[..., 3].view(np.uint32), g.npz["z"].view(np.uint32)), "z differs"
    assert np.array_equal(out[..., :3].view(np.uint32), g.npz["rgb"].view(np.uint32)), "linear RGB differs"
    assert (st["primary_rays"], st["primary_hits"], st["secondary_rays"], st["shadow_rays"]) == (
        g.meta["primary"], g.meta["primary_hits"], g.meta["secondary"], g.meta["shadow"])
    rgb8, _, zimg = orc.postprocess(out)
    assert np.array_equal(rgb8, g.npz["result_u8"]) and np.array_equal(zimg, g.npz["zbuffer_u8"])
    assert not np.isnan(out).any()


@pytest.mark.parametrize("name", sorted(TAGS))
def test_the_loader_flattens_the_scene_as_the_reference_does(pkg, golden, xf_dir, name):
    """Negative, zero and overflowing scales through this repository's loader: the blob of the scene file equals, byte for byte, the
    one the reference's loader serialised (tm, itm with their NaN and infinities, pos)."""
    import gzip
    scene = pkg.Scene.from_xml(os.path.join(str(xf_dir), FILES[name]))
    assert scene.to_blob_bytes() == gzip.open(os.path.join(golden(TAGS[name]).dir, "scene.rtus.gz")).read()


# ==== non-vacuity ===================================================================================================================
@pytest.mark.parametrize("label", ALL)
def test_first_hits_back_faces_and_singular_nodes(pkg, orc, xf_dir, label):
    scene, n_plain = scene_of(pkg, xf_dir, label)
    rays, h = camera_hits(pkg, orc, scene)
    fam = ray_families(pkg, orc, scene, 1)
    hs = [(n, r, orc.trace_rays(scene, r, threads=8)) for n, r in fam]
    counts, behind = {}, {}
    for k in transformed(scene, n_plain):
        counts[k] = int((h["node"] == k).sum())
        behind[k] = {n: int(((g["node"] == k) & ((g["flags"] & orc.RAY_FRONT) == 0)).sum()) for n, _, g in [("camera", rays, h)] + hs}
    sing = [k for k in counts if singular(scene, k)]
    nan = int(np.isnan(orc.render(scene, W, H, threads=8)[0]).any(axis=2).sum())
    best = max(behind, key=lambda k: max(behind[k].values()))
    print("%s: first hits of camera rays per node under the class %s; singular %s; most hits from behind: node %d %s; %d NaN pixels" %
          (label, counts, sing, best, behind[best], nan))
    # a group scaled x = 1e25 takes its children's normals through an inverse of 1e25: their squared length overflows, the reference
    # normalises by infinity and shades NaN — results like any other (check_against), at 1467 pixels
    assert nan == 0 or label == "T3 S=x1e25"
    for k, n in counts.items():
        if k in sing:
            assert n == 0 and not any((g["node"] == k).any() for _, _, g in hs), "a singular node is hit"
        elif not label.startswith("T4"):  # (T4's plane scaled by 1e30 lies behind the camera: what matters is that it loads and is traversed)
            assert n >= 50, "node %d is the first hit of %d camera rays" % (k, n)
    if label.startswith("T4"):
        assert len(sing) >= 6
    else:
        assert max(max(v.values()) for v in behind.values()) >= 20


@pytest.mark.parametrize("label", sorted(SCENES))
def test_secondary_and_shadow_rays_at_the_nodes_under_the_class(pkg, orc, xf_dir, label):
    """Against the scene without them: the counters move by at least 200 each way a ray can leave from or arrive at such a node."""
    name, kw = SCENES[label]
    scene, _ = load(pkg, xf_dir, name, **kw)
    bare, _ = load(pkg, xf_dir, name, removed=True, **kw)
    a, sa = orc.render(scene, W, H, threads=8)
    b, sb = orc.render(bare, W, H, threads=8)
    moved = int((a.view(np.uint32) != b.view(np.uint32)).any(axis=2).sum())
    print("%s: secondary rays %d (%d without the nodes under the class), shadow rays %d (%d), %d pixels differ" %
          (label, sa["secondary_rays"], sb["secondary_rays"], sa["shadow_rays"], sb["shadow_rays"], moved))
    if label == "T3 S=x1e25":
        # its hit points carry NaN normals (test_first_hits_back_faces_and_singular_nodes): most fire no shadow ray and no child, so
        # the counters move by less; the nodes still shadow the floor and are seen by it
        assert abs(sa["secondary_rays"] - sb["secondary_rays"]) >= 200 and moved >= 400
    elif not label.startswith("T4"):
        assert abs(sa["secondary_rays"] - sb["secondary_rays"]) >= 200 and abs(sa["shadow_rays"] - sb["shadow_rays"]) >= 200 and moved >= 400
    else:
        rays = ("primary_rays", "primary_hits", "secondary_rays", "shadow_rays")
        assert moved == 0 and [sa[k] for k in rays] == [sb[k] for k in rays], "a singular node changes the image"


@pytest.mark.parametrize("label", [l for l in ALL if not l.startswith("T4")])
def test_hits_the_plain_near_margin_would_skip(pkg, orc, xf_dir, label):
    """Reported, not required: on the oracle's own hits, how many the node-level test with the margin 1e-4 max(wscale, |origin|) would
    skip (model_skips of tests/test_oracle_far.py) — camera rays and the surface rays R2 built on them. Below the switch that margin IS
    the device's: a positive count there would be a bug in where the switch sits."""
    scene, n_plain = scene_of(pkg, xf_dir, label)
    rays, h = camera_hits(pkg, orc, scene)
    hit = (h["flags"] & orc.RAY_HIT) != 0
    r2 = family_r2(pkg, rays, h, hit)
    r2 = r2[valid(r2)]
    h2 = orc.trace_rays(scene, r2, threads=8)
    m = model_far(scene)
    fig, worst_d, worst_near = {}, 0.0, 0.0
    for what, rr, hh in (("camera", rays, h), ("R2", r2, h2)):
        total = skipped = 0
        for k in transformed(scene, n_plain):
            on = hh["node"] == k
            total += int(on.sum())
            skipped += int((on & model_skips(scene, k, rr, hh["t"].astype(np.float64))).sum())
            if on.any():  # the reference's own line against the bound D(pm) of THE CULL MARGIN and against the plain margin
                dev = line_deviation(scene, k, rr[on], hh["t"][on].astype(np.float64))
                pm = np.abs(rr["org"][on].astype(np.float64)).max(axis=1)
                worst_d = max(worst_d, float((dev / (m["wnoise"] * (pm + m["omega"] + 1.0) * (pm + m["wscale"]))).max()))
                worst_near = max(worst_near, float((dev / (1e-4 * np.maximum(m["wscale"], pm))).max()))
        fig[what] = (total, skipped)
    print("%s: the reference's line is off by at most %.3g D(pm) and %.3g of the plain margin where it hits" % (label, worst_d, worst_near))
    print("%s: K %.4g, D(2 wscale) / (12e-4 wscale) = %.3g (far term %s); (hits on the nodes under the class, of those skipped by the plain margin): %s" %
          (label, m["K"], m["DP"] / (12e-4 * m["wscale"]), "on" if m["on"] else "off", fig))
    assert fig["camera"][0] >= 50 and fig["R2"][0] >= 50
    if label.startswith("T5"):
        assert m["on"] == (label == "T5 above")
    assert worst_d <= 1.0, "the reference's line leaves the caller's by more than the far term bounds"
    if not m["on"]:
        assert fig["camera"][1] == 0 and fig["R2"][1] == 0 and worst_near <= 1.0, "the plain margin loses a hit below the switch"


def test_the_occluder_lists_show_the_switch(pkg, xf_dir):
    """The restated constants against what the builders used, through rtu_debug_light_list: a list's slack is 1e-4 wlist, and
    wlist = wscale below the switch, wscale + 1e4 D(2 wscale) — thirteen times as much — just above it. Two scenes that differ by a
    fifth in one card's aspect therefore differ by far more than that in the number of list entries, and two scenes below it do not."""
    def entries(ratio):
        scene, _ = load(pkg, xf_dir, "T5", aspect=t5_aspect(pkg, xf_dir, ratio), file="t5_entries.xml")
        m = model_far(scene)
        lists = [pkg.light_list(scene, ls, 0) for ls in range(2)]
        return m, [None if l is None else len(l["entry_face"]) for l in lists]
    (m0, e0), (m1, e1), (m2, e2) = entries(0.7), entries(0.9), entries(1.1)
    print("T5: wlist / wscale and list entries at 0.7, 0.9, 1.1 of the switch: %.2f %s, %.2f %s, %.2f %s" %
          (m0["wlist"] / m0["wscale"], e0, m1["wlist"] / m1["wscale"], e1, m2["wlist"] / m2["wscale"], e2))
    assert not m0["on"] and not m1["on"] and m2["on"] and 10.0 < m2["wlist"] / m2["wscale"] < 16.0
    for a, b, c in zip(e0, e1, e2):
        assert a is not None and b is not None
        assert abs(a - b) <= 0.02 * a, "two scenes below the switch build different lists"
        assert c is None or c > 1.5 * b, "the list just above the switch is no wider than below it"
